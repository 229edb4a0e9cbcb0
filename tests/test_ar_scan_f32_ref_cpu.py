"""The operand sets of the f32 context-model scan (tests/ref_ar_scan_f32.py) checked on the CPU before sc2_ar_scan_f32 is held
to them (tests/test_gpu_ar_scan_f32.py): they do tell an f32 scan from one that rounds its weights to bf16.

Measured for this construction (seed 0, numpy's summation order): the f32 evaluation's largest |err| / bound is 0.0014 - 0.041 on
SMALL_SHAPES, the same evaluation on bf16-rounded weights 10.6 - 954."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_ar_scan as RA  # noqa: E402
import ref_ar_scan_f32 as RF  # noqa: E402


def _id(shape):
    return 'x'.join(str(v) for v in shape)


def _scan(case, weights, dtype):
    return RA.scan_ref(weights, case['p1'], case['y'], case['scale_table'], case['scale_bound'], dtype=dtype)


@pytest.mark.parametrize('shape', RA.SMALL_SHAPES, ids=_id)
def test_random_f32_weights_are_f32_and_never_bf16(shape):
    case, _ = RF.cached('random_f32', shape)
    bf, _ = RA.cached('random', shape)
    C1, C2 = RA.real_widths(shape[1], shape[2])
    for name in RF.MATRICES:
        w = case['weights'][name]
        assert np.array_equal(RF.f32_only(w), w), name
        assert w.shape == bf['weights'][name].shape
        assert np.array_equal(w != 0, bf['weights'][name] != 0), '{}: the zero padding moved'.format(name)
        assert RF.not_bf16(w)[w != 0].all(), '{}: a non-zero weight is a bf16 number'.format(name)
        # the same draw as the bf16 set, rounded less: half a bf16 ulp (2^-9 relative) apart at the most
        assert (np.abs(w - bf['weights'][name]) <= 2.0 ** -8 * np.abs(w)).all(), name
    assert not case['weights']['w1'][:, C1:].any() and not case['weights']['w2'][C1:].any() and not case['weights']['w2'][:, C2:].any()
    assert not case['weights']['w3'][C2:].any()
    for name in ('bc', 'b2', 'b3'):
        assert np.array_equal(case['weights'][name], bf['weights'][name]), name
    assert np.array_equal(case['p1'], bf['p1']) and np.array_equal(case['y'], bf['y'])


@pytest.mark.parametrize('shape', RA.SMALL_SHAPES, ids=_id)
def test_random_f32_preconditions_and_bound(shape):
    """Both LeakyReLU branches occur, and an f32 evaluation of the step (numpy's order) passes the assertion the kernel is held to."""
    case, ref = RF.cached('random_f32', shape)
    print(shape, RA.check_random_preconditions(case, ref))
    assert RA.assert_random(case, ref) < 1e-6
    ratio = RA.assert_random(case, _scan(case, case['weights'], np.float32))
    print('f32 evaluation {}: largest |err| / bound = {:.3g}'.format(_id(shape), ratio))
    assert 0 < ratio < 1


@pytest.mark.parametrize('shape', RA.SMALL_SHAPES, ids=_id)
def test_bf16_rounded_weights_leave_the_bound(shape):
    """The same f32 evaluation on the weights a bf16 scan would read: outside the bound of the f32 weights' float64 step."""
    case, _ = RF.cached('random_f32', shape)
    got = _scan(case, RF.bf16_weights(case['weights']), np.float32)
    ratio = RA.bound_ratio(got['gaussian_params'], RA.teacher_forced_ref(case['weights'], case['p1'], got['y_hat_pad']))
    print('bf16-rounded weights {}: largest |err| / bound = {:.3g}'.format(_id(shape), ratio))
    assert ratio > 1
    with pytest.raises(AssertionError, match='outside the bound'):
        RA.assert_random(case, got)


@pytest.mark.parametrize('matrix', RF.MATRICES)
def test_lowbits_case_turns_on_one_weight(matrix):
    case, ref = RF.cached('lowbits', matrix)
    M, _, _, H, W, B = case['shape']
    assert np.array_equal(ref['symbols'].reshape(B, H * W, M), case['symbols'])
    diff = case['symbols_bf16'] - case['symbols']
    assert set(np.unique(diff)) == {0, 1} and (diff[..., 1] == 0).all()
    assert int(diff[..., 0].sum()) == B * H * (W - 1 if matrix == 'wc' else W)
    means = ref['gaussian_params'][:, :, M]
    assert np.array_equal(means, diff[..., 0].astype(np.float64))            # exactly 1 where the weight's low bit counts
    # every value is an exact f32 number and an f32 evaluation reproduces the float64 one bit for bit
    RA.assert_exact(ref, ref)
    RA.assert_exact(_scan(case, case['weights'], np.float32), ref)
    # the named matrix rounded to bf16: the other symbols, mean 0 everywhere, the same y_hat
    rounded = _scan(case, RF.bf16_weights(case['weights'], [matrix]), np.float64)
    assert np.array_equal(rounded['symbols'].reshape(B, H * W, M), case['symbols_bf16'])
    assert not rounded['gaussian_params'][:, :, M].any()
    assert np.array_equal(rounded['y_hat_pad'], ref['y_hat_pad'])
    assert np.array_equal(rounded['indexes'], ref['indexes'])
    # rounding any OTHER matrix changes nothing: the case is about one weight
    others = [m for m in RF.MATRICES if m != matrix]
    RA.assert_exact(_scan(case, RF.bf16_weights(case['weights'], others), np.float64), ref)
