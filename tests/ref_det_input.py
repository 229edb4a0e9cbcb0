"""Restatement of sc2_det_input (include/sc2_bottleneck.h) in numpy: the detector's input transform of one planned sample, from its
8-bit [h,w,3] source to the normalised, resized [3,oh,ow] image.

* `det_input_f32`  -- the kernel's arithmetic operation by operation, every operation rounded once in float32.
* `det_input_f64`  -- the same transform with exact weights in float64 (index and weight from the exact rational source position).
* `delta(h, w, mean, std)` -- the bound of either float32 form against float64, derived, not tuned:
      2 * spacing_f32(max(h, w)) * R + 8 * 2^-24 * M
  R = max - min of the table, M its largest magnitude.  The first term: the source position `scale * (d + 0.5) - 0.5` carries up to
  one float32 spacing (at the magnitude of the side) of error per axis, which moves the weight by as much and the value by that times
  the range of the table.  The second term covers the roundings of the interpolation itself (three products and sums per axis pair,
  one table entry).
"""
import numpy as np

F = np.float32


def table_f32(mean, std):
    """nrm[c][b] = ((float(b) / 255) - mean[c]) / std[c], each operation rounded once in float32 -> f32 [3, 256]"""
    b = np.arange(256, dtype=F)
    unit = b / F(255)
    return np.stack([((unit - F(m)) / F(s)).astype(F) for m, s in zip(mean, std)])


def table_f64(mean, std):
    """the same table from the float32 mean / std the kernel is handed, in float64"""
    unit = np.arange(256, dtype=np.float64) / 255.0
    return np.stack([(unit - float(F(m))) / float(F(s)) for m, s in zip(mean, std)])


def axis_f32(n_in, n_out):
    """aten's upsample_bilinear2d source index and weight per output index (align_corners=False, no given scale), in float32"""
    d = np.arange(n_out, dtype=F)
    scale = F(n_in) / F(n_out)
    src = np.maximum((scale * (d + F(0.5))).astype(F) - F(0.5), F(0)).astype(F)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(F)).astype(F)
    return i0, i1, l1


def axis_f64(n_in, n_out):
    d = np.arange(n_out, dtype=np.float64)
    src = np.maximum((d + 0.5) * (float(n_in) / float(n_out)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def det_input_f32(src, oh, ow, flip, mean, std):
    """src u8 [h,w,3] -> f32 [3,oh,ow]: v = ly0 * (lx0 * p + lx1 * q) + ly1 * (lx0 * s + lx1 * t), every operation rounded once"""
    h, w, _ = src.shape
    nrm = table_f32(mean, std)
    j0, j1, ly1 = axis_f32(h, oh)
    i0, i1, lx1 = axis_f32(w, ow)
    if flip:
        i0, i1 = w - 1 - i0, w - 1 - i1
    ly0, lx0 = (F(1) - ly1).astype(F)[:, None], (F(1) - lx1).astype(F)[None, :]
    ly1, lx1 = ly1[:, None], lx1[None, :]
    out = np.empty((3, oh, ow), dtype=F)
    for c in range(3):
        plane = nrm[c][src[:, :, c]]
        p, q, s, t = plane[j0][:, i0], plane[j0][:, i1], plane[j1][:, i0], plane[j1][:, i1]
        top = ((lx0 * p).astype(F) + (lx1 * q).astype(F)).astype(F)
        bottom = ((lx0 * s).astype(F) + (lx1 * t).astype(F)).astype(F)
        out[c] = ((ly0 * top).astype(F) + (ly1 * bottom).astype(F)).astype(F)
    return out


def det_input_f64(src, oh, ow, flip, mean, std):
    h, w, _ = src.shape
    nrm = table_f64(mean, std)
    j0, j1, ly1 = axis_f64(h, oh)
    i0, i1, lx1 = axis_f64(w, ow)
    if flip:
        i0, i1 = w - 1 - i0, w - 1 - i1
    ly1, lx1 = ly1[:, None], lx1[None, :]
    out = np.empty((3, oh, ow), dtype=np.float64)
    for c in range(3):
        plane = nrm[c][src[:, :, c]]
        p, q, s, t = plane[j0][:, i0], plane[j0][:, i1], plane[j1][:, i0], plane[j1][:, i1]
        out[c] = (1.0 - ly1) * ((1.0 - lx1) * p + lx1 * q) + ly1 * ((1.0 - lx1) * s + lx1 * t)
    return out


def delta(h, w, mean, std):
    nrm = table_f64(mean, std)
    R, M = float(nrm.max() - nrm.min()), float(np.abs(nrm).max())
    return 2.0 * float(np.spacing(F(max(h, w)))) * R + 8.0 * 2.0 ** -24 * M


def batch_f32(sources, sizes, flips, mean, std, Hp, Wp):
    """the whole padded batch the kernel writes: f32 [n,3,Hp,Wp], +0.0 outside each sample's (oh, ow)"""
    out = np.zeros((len(sources), 3, Hp, Wp), dtype=F)
    for i, (src, (oh, ow), flip) in enumerate(zip(sources, sizes, flips)):
        out[i, :, :oh, :ow] = det_input_f32(src, oh, ow, flip, mean, std)
    return out
