"""float64 restatement of `sc2_seg_ce_forward` / `sc2_seg_ce_backward` (include/sc2_bottleneck.h): cross entropy of the bilinearly
resized logits (tests/ref_seg.py's `interpolate`: index and lambda from integers) and its gradient with respect to the low-resolution
logits by the explicit adjoint -- and the cases and the tolerance rule that tests/test_seg_loss_ref_cpu.py, tests/test_seg_loss_cpu.py
and tests/test_gpu_seg_loss.py share.

Tolerance rule, derived (not fitted).  M = max|x| over the finite logits, u = 2^-24 (f32 rounding to nearest: relative error <= u).

* tests/ref_seg.py: each resized value v carries at most 6 u M (four products and three sums with weights correct to one ulp).
* `lse - v_t` doubles that (12 u M) and adds the roundings of `m + logf(s)` and of the difference, each <= u (M + ln C).
* the exponent arguments `v - m` carry 12 u M and one rounding more (u * 2 M), a RELATIVE error of the terms of the class sum, which
  are <= 1 while the sum is >= 1: the logarithm moves by no more.
* the class sum: the issue's derivation counts C roundings (a two-pass sum).  The kernel makes ONE online pass, as specified: each
  class step is either `s += expf(v - m)` (one expf, one addition) or, when the maximum moves, `s = s * expf(m - v) + 1` (one expf,
  one product, one addition), so up to 3 rounding-size relative errors of s per class instead of 1-2, expf itself at <= 1 ulp.  That
  is the term the issue's expression dropped: 2 C becomes 4 C (C steps x (expf + product + addition), rounded up).
* logf and the remaining single roundings: a few ulp of a number <= M + ln C, inside the constants below.

  tol_p = u * (32 M + 4 C + 32)              per pixel, for loss_p and lse_p; the same for the mean (its float64 sum adds nothing
                                             visible; the one f32 rounding of the quotient is inside the 32), count * tol_p for the sum.

Gradient: dx[i,j] = g * sum_p w_p(i,j) (softmax_p - onehot_p).  A[i,j] = sum_p |w_p(i,j)| (times |grad_out_p| for reduction 'none') over
the valid pixels, K[i,j] the number of terms.  softmax = expf(v - lse) <= 1 with an argument error <= tol_p / u ulps, so each term
is off by at most tol_p * w; the weight product, the product with the term and the K additions (each rounding a partial sum <= A)
add (3 + K) u A; g (one division) and the final product add 2 u more, inside the 32:

  tol_dx[i,j] = g * A[i,j] * u * (32 M + 4 C + 32 + K[i,j])   (+ 2^-8 |ref| for a bf16 dx: one rounding to 8 bits)
"""
import functools

import numpy as np
import torch

from tests import ref_seg
from tests.ref_seg import axis, interpolate, formula_f32      # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
IGNORE = 255

# ref_seg.CASES and the PASCAL ratio (65 -> 513 is 9 -> 65 up to the image size)
CASES = list(ref_seg.CASES) + [(1, 21, (9, 9), (65, 65), 1.0, 108)]
CASE_IDS = ['{}x{}_{}x{}_to_{}x{}'.format(n, c, h, w, H, W) for n, c, (h, w), (H, W), _, _ in CASES]
_N_SHARED = len(ref_seg.CASES)


@functools.lru_cache(maxsize=None)
def case_logits(index, dtype_name):
    """the seeded logits of CASES[index], rounded to the dtype under test"""
    if index < _N_SHARED:
        return ref_seg.case_logits(index, dtype_name)
    n, c, (h, w), _, scale, seed = CASES[index]
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(seed)) * scale
    return x.to(getattr(torch, dtype_name))


@functools.lru_cache(maxsize=None)
def case_targets(index):
    """int64 targets [N,H,W] drawn from {0..C-1, 255, -1, C, C+3}, seeded, every value at least once"""
    if index < _N_SHARED:
        return ref_seg.case_targets(index)
    n, c, _, (H, W), _, seed = CASES[index]
    values = torch.tensor(list(range(c)) + [255, -1, c, c + 3], dtype=torch.int64)
    t = values[torch.randint(0, len(values), (n, H, W), generator=torch.Generator().manual_seed(seed + 1000))]
    t.view(-1)[:len(values)] = values
    return t


def axis_first(k, n_in, n_out):
    """the first output index whose i0 is >= k (0 for k <= 0, n_out for k >= n_in): the kernel's gather range, in integers"""
    if k <= 0:
        return 0
    if k >= n_in:
        return n_out
    num = (2 * k + 1) * n_out - n_in
    if num <= 0:
        return 0
    return min(-(-num // (2 * n_in)), n_out)


def classify(targets, num_classes, ignore_index=IGNORE):
    """-> (valid, bad) bool arrays: valid = 0 <= t < C and t != ignore_index; bad = neither valid nor ignore_index"""
    t = np.asarray(targets, dtype=np.int64)
    valid = (t >= 0) & (t < num_classes) & (t != ignore_index)
    return valid, ~valid & (t != ignore_index)


class Reference(object):
    """everything the kernels produce for one (logits, size, targets), in float64"""

    def __init__(self, x, size, targets, ignore_index=IGNORE):
        x64 = np.asarray(x.double() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
        self.x, self.size, self.ignore_index = x64, size, ignore_index
        n, c, h, w = x64.shape
        self.t = np.asarray(targets, dtype=np.int64)
        self.valid, self.bad = classify(self.t, c, ignore_index)
        v = interpolate(x64, size)
        m = v.max(1, keepdims=True)
        self.lse = (m + np.log(np.exp(v - m).sum(1, keepdims=True)))[:, 0]
        tc = np.where(self.valid, self.t, 0)
        vt = np.take_along_axis(v, tc[:, None], 1)[:, 0]
        self.pixel_loss = np.where(self.valid, self.lse - vt, 0.0)
        self.count = int(self.valid.sum())
        self.n_bad = int(self.bad.sum())
        self.loss_sum = float(self.pixel_loss.sum())
        with np.errstate(invalid='ignore', divide='ignore'):
            self.loss_mean = float(np.float64(self.loss_sum) / np.float64(self.count))
        onehot = np.zeros_like(v)
        np.put_along_axis(onehot, tc[:, None], 1.0, 1)
        self.residual = (np.exp(v - self.lse[:, None]) - onehot) * self.valid[:, None]      # d loss_p / d v[p,:] at valid pixels, else 0
        finite = np.abs(x64[np.isfinite(x64)])
        self.M = float(finite.max()) if finite.size else 0.0
        self.C = c
        self.tol_p = U * (32.0 * self.M + 4.0 * c + 32.0)

    def _adjoint(self, field):
        """field: [N,K,H,W] -> [N,K,h,w]: the transpose of `interpolate`, np.add.at with the four weights"""
        n, _, h, w = self.x.shape
        H, W = self.size
        y0, y1, ly = axis(h, H)
        x0, x1, lx = axis(w, W)
        ly, lx = ly[:, None], lx[None, :]
        out = np.zeros((n, field.shape[1], h, w))
        for ys, wy in ((y0, 1.0 - ly), (y1, ly)):
            for xs, wx in ((x0, 1.0 - lx), (x1, lx)):
                np.add.at(out, (slice(None), slice(None), ys[:, None], xs[None, :]), field * (wy * wx))
        return out

    def grad(self, reduction='mean', grad_out=1.0):
        """-> (dx [N,C,h,w], tol [N,1,h,w]) for the f32 kernel; grad_out: a number, or [N,H,W] for 'none'"""
        if reduction == 'none':
            gp = np.asarray(grad_out, dtype=np.float64)
            g = 1.0
        else:
            gp = np.ones(self.t.shape)
            g = float(grad_out) if reduction == 'sum' else (float(grad_out) / self.count if self.count else 0.0)
        dx = g * self._adjoint(self.residual * gp[:, None])
        A = self._adjoint((np.abs(gp) * self.valid)[:, None])
        K = self._count()
        tol = abs(g) * A * U * (32.0 * self.M + 4.0 * self.C + 32.0 + K)
        return dx, tol

    def _count(self):
        """K[n,0,i,j]: the number of (valid pixel, corner) contributions that land on source pixel (i,j)"""
        n, _, h, w = self.x.shape
        H, W = self.size
        y0, y1, _ = axis(h, H)
        x0, x1, _ = axis(w, W)
        out = np.zeros((n, 1, h, w))
        ones = self.valid[:, None].astype(np.float64)
        for ys in (y0, y1):
            for xs in (x0, x1):
                np.add.at(out, (slice(None), slice(None), ys[:, None], xs[None, :]), ones)
        return out


@functools.lru_cache(maxsize=None)
def case_reference(index, dtype_name):
    """the shared, read-only reference of CASES[index] at the logits of `dtype_name`"""
    return Reference(case_logits(index, dtype_name), CASES[index][3], case_targets(index).numpy())


def pascal_stage_config(num_iterations=3, num_epochs=2, module_wise=True, scheduling_step=1, wrapper_key='DictLossWrapper'):
    """a `train.stage2` block in the shape of configs/pascal_voc2012/supervised_compression/entropic_student/*.yaml, inline"""
    optimizer = {'key': 'SGD', 'kwargs': {'lr': 0.0025, 'momentum': 0.9, 'weight_decay': 0.0001}}
    if module_wise:
        optimizer['module_wise_kwargs'] = [{'module': 'backbone', 'kwargs': {}}, {'module': 'classifier', 'kwargs': {}},
                                           {'module': 'aux_classifier', 'kwargs': {'lr': 0.025}}]
    scheduler = {'key': 'poly_lr_scheduler', 'kwargs': {'num_iterations': num_iterations, 'num_epochs': num_epochs, 'power': 0.9}}
    if scheduling_step is not None:
        scheduler['scheduling_step'] = scheduling_step
    return {
        'num_epochs': num_epochs,
        'teacher': {'sequential': [], 'forward_hook': {'input': [], 'output': []}, 'requires_grad': False},
        'student': {'sequential': [], 'frozen_modules': [], 'forward_hook': {'input': [], 'output': []}, 'requires_grad': True},
        'optimizer': optimizer,
        'scheduler': scheduler,
        'criterion': {'key': 'WeightedSumLoss', 'kwargs': {'sub_terms': {'ce': {
            'criterion': {'key': 'CrossEntropyLoss', 'kwargs': {'reduction': 'mean', 'ignore_index': 255}},
            'criterion_wrapper': {'key': wrapper_key, 'kwargs': {
                'input': {'is_from_teacher': False, 'module_path': '.', 'io': 'output'},
                'target': {'uses_label': True},
                'weights': {'out': 1.0, 'aux': 0.5}}},
            'weight': 1.0}}}},
    }


class TinyBackbone(torch.nn.Module):
    """stand-in feature extractor: {'out': [N,6,h/4,w/4], 'aux': [N,4,h/2,w/2]}"""

    def __init__(self):
        super().__init__()
        self.aux = torch.nn.Conv2d(3, 4, 3, stride=2, padding=1)
        self.out = torch.nn.Conv2d(4, 6, 3, stride=2, padding=1)

    def get_aux_module(self):      # (no entropy model: the stage has no auxiliary loss to step)
        return None

    def forward(self, x):
        a = torch.tanh(self.aux(x))
        return {'out': torch.tanh(self.out(a)), 'aux': a}


def tiny_seg_model(num_classes=5, seed=3):
    """a `BaseSegmentationModel` over TinyBackbone with 1x1-conv heads (f32, any device)"""
    from sc2bench_amd.dense import BaseSegmentationModel
    torch.manual_seed(seed)
    return BaseSegmentationModel(TinyBackbone(), torch.nn.Conv2d(6, num_classes, 1), torch.nn.Conv2d(4, num_classes, 1))


def tiny_batch(num_classes=5, seed=4, size=(21, 27)):
    """-> (images [2,3,H,W], targets [2,H,W] with 255 among them)"""
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(2, 3, size[0], size[1], generator=g)
    targets = torch.randint(0, num_classes + 1, (2, size[0], size[1]), generator=g)
    targets[targets == num_classes] = IGNORE
    return images, targets


def assert_close(got, want, tol, what):
    """element-wise |got - want| <= tol (NaN never passes); prints the worst ratio before it asserts"""
    got = np.asarray(got.detach().double().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    print('{}: max err {:.3e}, worst err / tol {:.3f}'.format(what, float(np.nanmax(err)) if err.size else 0.0, worst))
    assert not np.isnan(got).any(), '{}: NaN in the result'.format(what)
    bad = err > tol
    assert not bad.any(), '{}: {} elements outside the tolerance, first at {} (err {:.3e}, tol {:.3e})'.format(
        what, int(bad.sum()), np.argwhere(bad)[0], err[bad][0], tol[bad][0])
