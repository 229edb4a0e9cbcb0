"""Pillow's two resizes of 8-bit images, restated in numpy, and the PASCAL augmentation chain built from them: what
csrc/seg_augment.hip computes.  tests/test_pil_resize_ref_cpu.py proves the two resizes against Pillow itself, byte for byte.

Bilinear (`ImagingResample`, 8 bits per channel).  Per axis n_in -> n_out, all in float64, every operation rounded once:
    scale = n_in / n_out;  filterscale = support = max(scale, 1);  ksize = 2 * ceil(support) + 1
    center = (xx + 0.5) * scale;  first = max(int(center - support + 0.5), 0);  count = min(int(center + support + 0.5), n_in) - first
    w_x = max(0, 1 - |(x + first - center + 0.5) * (1 / filterscale)|),  summed left to right, each divided by the sum
    k_x = int(0.5 + w_x * 2^22)
A pass is clip((2^21 + sum(pixel * k_x)) >> 22, 0, 255); the horizontal pass runs first and gives 8-bit values, the vertical pass runs
on those; a pass whose two lengths are equal is skipped.
Nearest (`ImagingScaleAffine`).  Per axis the source index of output i is int(xo), xo = a * 0.5 for i = 0 and xo += a afterwards,
a = n_in / n_out: a running float64 sum, not i * a.
"""
import functools
import math

import numpy as np

PRECISION_BITS = 22


@functools.lru_cache(maxsize=None)
def coeffs(n_in, n_out):
    """-> (bounds int [n_out, 2]: first source index and count; k int64 [n_out, ksize]: the fixed-point coefficients, 0 behind count)"""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int64)
    k = np.zeros((n_out, ksize), np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n_in) - first
        weights = []
        for x in range(count):
            v = abs((x + first - center + 0.5) * inv)
            weights.append(1.0 - v if v < 1.0 else 0.0)
        total = 0.0
        for v in weights:
            total += v
        for x in range(count):
            p = weights[x] / total if total != 0.0 else weights[x]
            k[xx, x] = int(-0.5 + p * (1 << PRECISION_BITS)) if p < 0 else int(0.5 + p * (1 << PRECISION_BITS))
        bounds[xx] = first, count
    return bounds, k


def _pass(a, n_out):
    """resamples axis 1 of a uint8 [R, n_in, C]"""
    bounds, k = coeffs(a.shape[1], n_out)
    out = np.empty((a.shape[0], n_out, a.shape[2]), np.uint8)
    for xx, (first, count) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + (a[:, first:first + count, :].astype(np.int64) * k[xx, :count][None, :, None]).sum(1)
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_bilinear(a, nh, nw):
    """uint8 [h, w, C] -> uint8 [nh, nw, C]: `Image.fromarray(a).resize((nw, nh), Image.BILINEAR)`"""
    h, w, _ = a.shape
    if nw != w:
        a = _pass(a, nw)
    if nh != h:
        a = _pass(a.transpose(1, 0, 2), nh).transpose(1, 0, 2)
    return np.ascontiguousarray(a)


@functools.lru_cache(maxsize=None)
def nearest_table(n_in, n_out):
    step = n_in / n_out
    xo = step * 0.5
    table = []
    for _ in range(n_out):
        table.append(int(xo))
        xo += step
    return np.array(table, dtype=np.int64)


def resize_nearest(t, nh, nw):
    """uint8 [h, w] -> uint8 [nh, nw]: `Image.fromarray(t).resize((nw, nh), Image.NEAREST)`"""
    h, w = t.shape
    return np.ascontiguousarray(t[nearest_table(h, nh)][:, nearest_table(w, nw)])


def augment(image, mask, nh, nw, flip, top, left, out_h, out_w, pad_h, pad_w, mean, std):
    """The chain of one sample: resize to nh x nw, flip, pad right / bottom to pad_h x pad_w (image 0, mask 255), crop out_h x out_w at
    (top, left), ToTensor, Normalize -> (float32 [3, out_h, out_w], int64 [out_h, out_w]); float32 arithmetic as torch's."""
    img, msk = resize_bilinear(image, nh, nw), resize_nearest(mask, nh, nw)
    if flip:
        img, msk = img[:, ::-1], msk[:, ::-1]
    img_p = np.zeros((pad_h, pad_w, 3), np.uint8)
    msk_p = np.full((pad_h, pad_w), 255, np.uint8)
    img_p[:nh, :nw], msk_p[:nh, :nw] = img, msk
    img_c, msk_c = img_p[top:top + out_h, left:left + out_w], msk_p[top:top + out_h, left:left + out_w]
    assert img_c.shape[:2] == (out_h, out_w)
    x = img_c.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    x = (x - np.asarray(mean, np.float32).reshape(3, 1, 1)) / np.asarray(std, np.float32).reshape(3, 1, 1)
    return x.astype(np.float32), msk_c.astype(np.int64)


def table_entries(n_in, n_out, origin, length, ext, flip=False):
    """The kernel's table of one axis as the workspace holds it: int32 [length, 12] = first, count, nine coefficients, nearest index, for
    the window positions origin .. origin + length - 1; zero where a position shows no resized pixel."""
    bounds, k = coeffs(n_in, n_out)
    near = nearest_table(n_in, n_out)
    out = np.zeros((length, 12), np.int32)
    for o in range(length):
        r = origin + o
        if o < ext and r < n_out:
            j = n_out - 1 - r if flip else r
            out[o, 0:2] = bounds[j]
            out[o, 2:2 + min(k.shape[1], 9)] = k[j, :9]
            out[o, 11] = near[j]
    return out
