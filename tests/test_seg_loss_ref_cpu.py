"""tests/ref_seg_loss.py, the float64 restatement of the segmentation training loss, against torch's own ops in float64, on hand-worked
cases, and its tolerance rule against the f32 evaluation of the stated formula on torch CPU ops (no kernel here)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ref_seg_loss as RL

INDEXES = range(len(RL.CASES))


def _torch_side(x, size, targets, reduction='mean', dtype=torch.float64):
    """F.interpolate + F.cross_entropy with autograd; out-of-range targets mapped to ignore_index (torch would assert on them)"""
    c = x.shape[1]
    t = targets.clone()
    t[(t < 0) | (t >= c)] = RL.IGNORE
    xx = x.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(F.interpolate(xx, size=size, mode='bilinear', align_corners=False), t, ignore_index=RL.IGNORE, reduction=reduction)
    return xx, loss


@pytest.mark.parametrize('index', INDEXES, ids=RL.CASE_IDS)
def test_restatement_equals_torch_in_float64(index):
    size = RL.CASES[index][3]
    x, targets = RL.case_logits(index, 'float32'), RL.case_targets(index)
    ref = RL.case_reference(index, 'float32')
    assert ref.n_bad > 0 and 0 < ref.count < targets.numel()
    for reduction, want in (('mean', ref.loss_mean), ('sum', ref.loss_sum)):
        xx, loss = _torch_side(x, size, targets, reduction)
        loss.backward()
        assert abs(loss.item() - want) <= 1e-12 * max(1.0, abs(want)), (reduction, loss.item(), want)
        dx, _ = ref.grad(reduction)
        assert np.abs(xx.grad.numpy() - dx).max() <= 1e-12, reduction
    # reduction 'none' with a per-pixel gradient
    xx, loss = _torch_side(x, size, targets, 'none')
    gp = torch.rand(loss.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64) - 0.3
    loss.backward(gp)
    assert np.abs(loss.detach().numpy() - ref.pixel_loss).max() <= 1e-12
    assert np.abs(xx.grad.numpy() - ref.grad('none', gp.numpy())[0]).max() <= 1e-12


def test_one_source_pixel_gives_a_uniform_gradient():
    """1x1 -> HxW: every output pixel reads the one source pixel with weight 1, so dx = mean over valid pixels of softmax - onehot"""
    x = torch.tensor([0.5, -1.0, 2.0]).view(1, 3, 1, 1)
    targets = torch.tensor([[[0, 1, 2, 255], [2, 2, -1, 7]]])
    ref = RL.Reference(x, (2, 4), targets.numpy())
    assert ref.count == 5 and ref.n_bad == 2
    p = np.exp(x.numpy().reshape(3).astype(np.float64))
    p /= p.sum()
    want = (5 * p - np.array([1.0, 1.0, 3.0])) / 5
    dx, tol = ref.grad('mean')
    assert np.abs(dx.reshape(3) - want).max() <= 1e-15 and dx.shape == (1, 3, 1, 1)
    assert np.allclose(ref.lse, np.log(np.exp(x.numpy().reshape(3).astype(np.float64)).sum())) and tol.shape == (1, 1, 1, 1)


def test_one_class_gives_zero_loss_and_gradient():
    ref = RL.case_reference(4, 'float32')
    assert ref.C == 1 and ref.count > 0
    assert ref.loss_sum == 0.0 and not ref.pixel_loss.any()
    assert not ref.grad('sum')[0].any()


def test_all_ignored_gives_nan_loss_and_zero_gradient():
    x = RL.case_logits(0, 'float32')
    targets = torch.full_like(RL.case_targets(0), RL.IGNORE)
    ref = RL.Reference(x, RL.CASES[0][3], targets.numpy())
    assert ref.count == 0 and ref.n_bad == 0 and np.isnan(ref.loss_mean) and ref.loss_sum == 0.0
    dx, tol = ref.grad('mean')
    assert not dx.any() and not tol.any()
    xx, loss = _torch_side(x, RL.CASES[0][3], targets)
    loss.backward()
    assert torch.isnan(loss) and not xx.grad.any()


@pytest.mark.parametrize('n_in,n_out', [(1, 1), (1, 7), (9, 67), (11, 83), (8, 5), (8, 3), (17, 130), (4, 9), (65, 513), (3, 3), (100, 7)])
def test_gather_ranges_cover_exactly_the_footprints(n_in, n_out):
    """rows d with i0(d) in {i-1, i} are axis_first(i-1) .. axis_first(i+1) - 1, and no other row touches source row i"""
    i0, i1, _ = RL.axis(n_in, n_out)
    assert (np.diff(i0) >= 0).all()
    for i in range(n_in):
        lo, hi = RL.axis_first(i - 1, n_in, n_out), RL.axis_first(i + 1, n_in, n_out)
        touching = np.nonzero((i0 == i) | (i1 == i))[0]
        assert 0 <= lo <= hi <= n_out
        assert all(lo <= d < hi for d in touching), (i, lo, hi, touching)
        inside = np.arange(lo, hi)
        assert ((i0[inside] >= i - 1) & (i0[inside] <= i) & (i1[inside] <= i + 1)).all()      # what the kernel's LDS tile holds


@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
@pytest.mark.parametrize('index', INDEXES, ids=RL.CASE_IDS)
def test_tolerance_rule_holds_for_the_f32_formula_on_cpu(index, dtype_name):
    """formula_f32 + f32 logsumexp + autograd on torch CPU ops: the rule of the module docstring, checked without the kernel"""
    size = RL.CASES[index][3]
    x, targets = RL.case_logits(index, dtype_name), RL.case_targets(index)
    ref = RL.case_reference(index, dtype_name)
    xx = x.float().clone().requires_grad_(True)
    v = RL.formula_f32(xx, size)
    assert v.dtype == torch.float32
    lse = torch.logsumexp(v, 1)
    valid = torch.from_numpy(ref.valid)
    tc = torch.where(valid, targets, torch.zeros_like(targets))
    pixel = torch.where(valid, lse - v.gather(1, tc[:, None])[:, 0], torch.zeros_like(lse))
    what = '{} {}'.format(RL.CASE_IDS[index], dtype_name)
    RL.assert_close(lse, ref.lse, ref.tol_p, what + ' lse')
    RL.assert_close(pixel, ref.pixel_loss, ref.tol_p, what + ' pixel loss')
    mean = pixel.double().sum() / ref.count
    RL.assert_close(mean.float(), ref.loss_mean, ref.tol_p, what + ' mean')
    (pixel.sum() / ref.count).backward()
    dx, tol = ref.grad('mean')
    RL.assert_close(xx.grad, dx, tol, what + ' dx')
