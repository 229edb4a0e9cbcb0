"""float64 restatement of `sc2_seg_predict` (include/sc2_bottleneck.h): bilinear resize with align_corners=False whose source index
and weight come from integers, first-maximum labels with NaN as the maximum, the confusion matrix of SegEvaluator.update -- and the
shared cases, tolerance rule and f32 formula evaluation that tests/test_seg_ref_cpu.py and tests/test_gpu_seg_predict.py use.

The label rule of the GPU tests: the kernel's labels must equal this file's at every pixel whose float64 top-2 margin exceeds
tol = 2^-19 * max|x|.  Four products and three sums with weights correct to one ulp give at most about 6 * 2^-24 * max|x| per value;
doubled for a difference of two values that is 2^-20.4 * max|x|, and the tolerance leaves one extra bit.  At most 1e-3 of a case's
pixels may fall under the tolerance (asserted: a rule that excludes more checks too little).
"""
import functools

import numpy as np
import torch

TOL_FACTOR = 2.0 ** -19
EXCLUDED_CAP = 1e-3

# N, C, (h, w), (H, W), scale of the random normal logits, seed
CASES = [
    (2, 21, (9, 11), (67, 83), 1.0, 101),
    (3, 5, (1, 1), (7, 9), 1.0, 102),
    (2, 21, (5, 7), (33, 50), 8.0, 103),
    (1, 64, (3, 4), (20, 29), 1.0, 104),
    (1, 1, (4, 4), (9, 9), 1.0, 105),          # one class: every label is 0
    (2, 7, (8, 8), (5, 3), 1.0, 106),          # downsampling
    (1, 21, (17, 17), (129, 130), 1.0, 107),   # W is a multiple of no tile
]
CASE_IDS = ['{}x{}_{}x{}_to_{}x{}'.format(n, c, h, w, H, W) for n, c, (h, w), (H, W), _, _ in CASES]


def axis(n_in, n_out):
    """-> (i0, i1 int64 [n_out], lambda float64 [n_out]): t = (2d+1)*n_in - n_out is the source coordinate times 2*n_out"""
    d = np.arange(n_out, dtype=np.int64)
    t = (2 * d + 1) * n_in - n_out
    pos = t > 0
    den = 2 * n_out
    i0 = np.where(pos, t // den, 0)
    lam = np.where(pos, (t % den).astype(np.float64) / float(den), 0.0)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, lam


def interpolate(x, size):
    """x: [N,C,h,w] tensor or array -> float64 array [N,C,H,W]: (1-ly)*((1-lx)*a + lx*b) + ly*((1-lx)*c + lx*d)"""
    x = np.asarray(x.double() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    H, W = size
    y0, y1, ly = axis(x.shape[2], H)
    x0, x1, lx = axis(x.shape[3], W)
    ly, lx = ly[:, None], lx[None, :]
    a, b = x[:, :, y0][:, :, :, x0], x[:, :, y0][:, :, :, x1]
    c, d = x[:, :, y1][:, :, :, x0], x[:, :, y1][:, :, :, x1]
    with np.errstate(invalid='ignore'):      # (0 * inf = NaN is the specification's, not an accident)
        return (1.0 - ly) * ((1.0 - lx) * a + lx * b) + ly * ((1.0 - lx) * c + lx * d)


def labels_and_margin(v):
    """v: float [N,C,H,W] -> (int64 labels [N,H,W]: the first class holding the maximum, a NaN above every number and the first NaN
    final; float64 margin [N,H,W]: largest minus second largest value, +inf where a NaN decides or there is one class)"""
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v)
    any_nan = nan.any(1)
    clean = np.where(nan, -np.inf, v)
    labels = np.where(any_nan, nan.argmax(1), clean.argmax(1)).astype(np.int64)      # (argmax: the first of equal entries)
    if v.shape[1] == 1:
        return labels, np.full(labels.shape, np.inf)
    top = np.sort(clean, axis=1)
    with np.errstate(invalid='ignore'):
        margin = top[:, -1] - top[:, -2]
    margin = np.where(any_nan | np.isnan(margin), np.inf, margin)
    return labels, margin


def predict(x, size):
    """-> (labels, margin, values) of the float64 restatement"""
    v = interpolate(x, size)
    labels, margin = labels_and_margin(v)
    return labels, margin, v


def confusion(targets, labels, num_classes, mat=None):
    """mat[t, p] += 1 for every pixel with 0 <= t < num_classes (int64 [C,C]); a plain bincount"""
    t = np.asarray(targets).reshape(-1).astype(np.int64)
    p = np.asarray(labels).reshape(-1).astype(np.int64)
    keep = (t >= 0) & (t < num_classes)
    out = np.bincount(num_classes * t[keep] + p[keep], minlength=num_classes ** 2).reshape(num_classes, num_classes).astype(np.int64)
    return out if mat is None else mat + out


def miou(mat):
    h = np.asarray(mat, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.mean(np.diag(h) / (h.sum(1) + h.sum(0) - np.diag(h)) * 100.0))


def tolerance(x):
    """2^-19 * max|x| over the finite entries of the real classes"""
    a = np.abs(np.asarray(x.double() if isinstance(x, torch.Tensor) else x, dtype=np.float64))
    a = a[np.isfinite(a)]
    return TOL_FACTOR * (float(a.max()) if a.size else 0.0)


def assert_labels(got, x, size, what=''):
    """the label rule of the module docstring; -> the number of excluded pixels"""
    want, margin, _ = predict(x, size)
    got = np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got)
    assert got.shape == want.shape and got.dtype == np.int64, (what, got.shape, got.dtype)
    decided = margin > tolerance(x)
    excluded = int((~decided).sum())
    print('{}: {} of {} pixels under the tolerance, {} labels differ among the others'.format(
        what, excluded, decided.size, int(((got != want) & decided).sum())))
    assert excluded <= EXCLUDED_CAP * decided.size, '{}: {} of {} pixels excluded'.format(what, excluded, decided.size)
    bad = (got != want) & decided
    assert not bad.any(), '{}: {} labels differ at decided pixels, first at {}'.format(what, int(bad.sum()), np.argwhere(bad)[0])
    return excluded


def formula_f32(x, size):
    """The stated formula in f32, one rounding per operation (torch CPU ops do not fuse): what the kernel evaluates.
    x: f32 or bf16 tensor [N,C,h,w] -> f32 tensor [N,C,H,W]"""
    x = x.float()
    H, W = size

    def ax(n_in, n_out):
        i0, i1, _ = axis(n_in, n_out)
        t = (2 * np.arange(n_out, dtype=np.int64) + 1) * n_in - n_out
        num = torch.from_numpy(np.where(t > 0, t % (2 * n_out), 0)).to(torch.float32)
        return torch.from_numpy(i0), torch.from_numpy(i1), num / torch.tensor(float(2 * n_out), dtype=torch.float32)
    y0, y1, ly = ax(x.shape[2], H)
    x0, x1, lx = ax(x.shape[3], W)
    ly, lx = ly[:, None], lx[None, :]
    hy, hx = 1.0 - ly, 1.0 - lx
    a, b = x[:, :, y0][:, :, :, x0], x[:, :, y0][:, :, :, x1]
    c, d = x[:, :, y1][:, :, :, x0], x[:, :, y1][:, :, :, x1]
    return hy * (hx * a + lx * b) + ly * (hx * c + lx * d)


@functools.lru_cache(maxsize=None)
def case_logits(index, dtype_name):
    """the seeded logits of CASES[index], rounded to the dtype under test (the restatement then reads exactly those values)"""
    n, c, (h, w), _, scale, seed = CASES[index]
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(seed)) * scale
    return x.to(getattr(torch, dtype_name))


def case_targets(index, extra=()):
    """int64 targets [N,H,W] drawn from {0..C-1, 255, -1, C, C+3} (+ `extra`), seeded"""
    n, c, _, (H, W), _, seed = CASES[index]
    values = torch.tensor(list(range(c)) + [255, -1, c, c + 3] + list(extra), dtype=torch.int64)
    pick = torch.randint(0, len(values), (n, H, W), generator=torch.Generator().manual_seed(seed + 1000))
    t = values[pick]
    if t.numel() >= len(values):      # every value at least once, also in the smallest case
        t.view(-1)[:len(values)] = values
    return t
