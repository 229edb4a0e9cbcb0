"""Float64 / numpy restatement of the two kernels of csrc/rcnn_input.hip, written from the formulas of include/sc2_bottleneck.h.

* `resize_ref`: bilinear, align_corners=False, EXACT weights -- `src = max((d + 0.5) * in / out - 0.5, 0)` and the interpolation in
  float64 -- and `v * 255` as float64, not truncated.
* `check_resize`: the rule a byte image is held against.  A byte g is right if `g == floor(v255)`; where `|v255 - round(v255)| <=
  delta` it is also right if `g in {round(v255) - 1, round(v255)}`: an implementation in f32 may land on either side of an integer
  that the exact value all but touches.
* `resize_delta(H, W)`: `255 * 2 * spacing_f32(max(H, W)) + 2e-4`.  The first term is one f32 spacing of error in each axis's source
  index (its magnitude is below the input side) times the value range; the second the four roundings of the interpolation
  (4 * 2^-24 * 255 = 6e-5) with room.
* `normalize_pad_ref`: numpy float32, operation by operation: `((p / 255) - mean) / std` inside, +0.0 outside.
"""
import numpy as np

MARGIN_CAP = 0.05       # at most this share of a random-input case's pixels may be decided by the margin clause


def _axis(n_in, n_out):
    d = np.arange(n_out, dtype=np.float64)
    src = np.maximum((d + 0.5) * (float(n_in) / float(n_out)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def resize_ref(x, oh, ow):
    """x: [C,H,W] array of floats -> float64 [C,oh,ow]: the exact-weight bilinear value times 255."""
    x = np.asarray(x, dtype=np.float64)
    _, H, W = x.shape
    y0, y1, ly0, ly1 = _axis(H, oh)
    x0, x1, lx0, lx1 = _axis(W, ow)
    top = x[:, y0][:, :, x0] * lx0 + x[:, y0][:, :, x1] * lx1
    bot = x[:, y1][:, :, x0] * lx0 + x[:, y1][:, :, x1] * lx1
    return (top * ly0[None, :, None] + bot * ly1[None, :, None]) * 255.0


def resize_delta(H, W):
    return 255.0 * 2.0 * float(np.spacing(np.float32(max(H, W)))) + 2e-4


def check_resize(got_u8, v255, delta):
    """-> (number of wrong bytes, share of the pixels decided by the margin clause)."""
    g = np.asarray(got_u8).astype(np.int64)
    v255 = np.asarray(v255, dtype=np.float64)
    assert g.shape == v255.shape
    exact = g == np.floor(v255).astype(np.int64)
    r = np.rint(v255)
    near = np.abs(v255 - r) <= delta
    by_margin = ~exact & near & ((g == r.astype(np.int64)) | (g == r.astype(np.int64) - 1))
    wrong = ~exact & ~by_margin
    return int(wrong.sum()), float(by_margin.mean())


def normalize_pad_ref(pixels_u8, mean, std, Hp, Wp):
    """pixels: uint8 [C,h,w] -> float32 [C,Hp,Wp]"""
    p = np.asarray(pixels_u8)
    assert p.dtype == np.uint8
    C, h, w = p.shape
    assert Hp >= h and Wp >= w
    out = np.zeros((C, Hp, Wp), dtype=np.float32)
    unit = p.astype(np.float32) / np.float32(255.0)
    m = np.asarray(mean, dtype=np.float32).reshape(C, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(C, 1, 1)
    out[:, :h, :w] = (unit - m) / s
    return out
