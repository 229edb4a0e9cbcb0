"""tests/ref_seg.py, the float64 restatement of `sc2_seg_predict`, against torch's own bilinear resize in float64 -- and, for every
seeded case of the GPU tests, that an f32 evaluation of the stated formula stays inside the label rule the GPU tests apply."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ref_seg

SIZES = [((1, 1), (7, 9)), ((9, 11), (67, 83)), ((5, 7), (33, 50)), ((8, 8), (5, 3))]


@pytest.mark.parametrize('hw,size', SIZES)
def test_restatement_matches_torch_float64(hw, size):
    x = torch.randn(2, 6, hw[0], hw[1], generator=torch.Generator().manual_seed(hw[0] * 100 + hw[1]), dtype=torch.float64)
    want = F.interpolate(x, size=size, mode='bilinear', align_corners=False)
    labels, margin, got = ref_seg.predict(x, size)
    err = np.abs(got - want.numpy()).max() / want.abs().max().item()
    print('{} -> {}: max error relative to max|value| {:.3g}, smallest margin {:.3g}'.format(hw, size, err, margin.min()))
    assert np.allclose(got, want.numpy(), rtol=1e-12, atol=1e-12 * want.abs().max().item())
    assert margin.min() > 1e-9       # (no pixel of these seeds is near a tie: equal labels are then a property of the values)
    assert np.array_equal(labels, want.argmax(1).numpy())


def test_axis_rule():
    i0, i1, lam = ref_seg.axis(1, 7)
    assert not i0.any() and not i1.any()       # (a one-pixel axis: both neighbours are pixel 0 whatever the weight)
    i0, i1, lam = ref_seg.axis(4, 8)       # source coordinate (d + 0.5) / 2 - 0.5
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and i1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert lam.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25]
    i0, i1, lam = ref_seg.axis(8, 3)       # downsampling: (d + 0.5) * 8 / 3 - 0.5
    assert i0.tolist() == [0, 3, 6] and i1.tolist() == [1, 4, 7] and np.allclose(lam, [5 / 6, 0.5, 1 / 6], rtol=1e-15)


def test_labels_first_maximum_and_nan():
    v = np.zeros((1, 4, 1, 5))
    v[0, :, 0, 0] = [1, 3, 3, 2]                       # a tie: the lower index
    v[0, :, 0, 1] = [1, np.nan, 5, np.nan]             # NaN above every number, the first NaN
    v[0, :, 0, 2] = [np.nan, 9, 9, 9]
    v[0, :, 0, 3] = [-1, -2, -3, -0.5]
    v[0, :, 0, 4] = [0, 0, 0, 0]
    labels, margin = ref_seg.labels_and_margin(v)
    assert labels[0, 0].tolist() == [1, 1, 0, 3, 0]
    assert margin[0, 0].tolist() == [0.0, np.inf, np.inf, 0.5, 0.0]
    assert np.array_equal(labels, torch.from_numpy(v).argmax(1).numpy())      # torch.argmax has the same rule


def test_confusion_matches_evaluator_formula(S):
    c = 6
    g = torch.Generator().manual_seed(5)
    values = torch.tensor(list(range(c)) + [255, -1, c, c + 3])
    targets = values[torch.randint(0, len(values), (3, 9, 10), generator=g)]
    labels = torch.randint(0, c, (3, 9, 10), generator=g)
    ev = S.dense.SegEvaluator(c)
    ev.update(targets.flatten(), labels.flatten())
    got = ref_seg.confusion(targets.numpy(), labels.numpy(), c)
    assert np.array_equal(got, ev.mat.numpy()) and got.sum() < targets.numel()
    ev.update(targets.flatten(), labels.flatten())
    assert np.array_equal(ref_seg.confusion(targets.numpy(), labels.numpy(), c, mat=got), ev.mat.numpy())
    _, _, iou = ev.compute()
    assert abs(ref_seg.miou(ev.mat.numpy()) - iou.mean().item()) < 1e-4


@pytest.mark.parametrize('index', range(len(ref_seg.CASES)), ids=ref_seg.CASE_IDS)
@pytest.mark.parametrize('dtype', ['bfloat16', 'float32'])
def test_f32_formula_stays_inside_the_label_rule(index, dtype):
    """the seeds the GPU tests use: the formula evaluated in f32 gives the restatement's label wherever the margin exceeds the
    tolerance, and the tolerance excludes at most 1e-3 of the pixels"""
    x = ref_seg.case_logits(index, dtype)
    size = ref_seg.CASES[index][3]
    got = ref_seg.formula_f32(x, size).argmax(1).numpy()
    ref_seg.assert_labels(got, x, size, what='f32 formula, case {} {}'.format(ref_seg.CASE_IDS[index], dtype))
    if ref_seg.CASES[index][1] == 1:
        assert not got.any()


@pytest.mark.parametrize('index', [0, 2, 6])
@pytest.mark.parametrize('dtype', ['bfloat16', 'float32'])
def test_f32_formula_on_the_all_negative_variant(index, dtype):
    """the logits of the GPU tests' pad-channel cases (every real logit negative), same rule"""
    x = -(ref_seg.case_logits(index, dtype).abs() + 0.5)
    size = ref_seg.CASES[index][3]
    ref_seg.assert_labels(ref_seg.formula_f32(x, size).argmax(1).numpy(), x, size, what='f32 formula, negative case {} {}'.format(index, dtype))
