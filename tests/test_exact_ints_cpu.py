"""The integer-operand helper (tests/exact_ints.py) itself, without a GPU: its f32 and f64 references against an int64 einsum, the
narrow operand rule at the K values the GPU cases use, the exactness bound, the one rounding of `cast`, the failure report of
`assert_bits_equal`, and the guard-band arena."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import exact_ints as E  # noqa: E402


@pytest.mark.parametrize('kind', ['wide', 'narrow'])
@pytest.mark.parametrize('cin,cout,k,stride,pad,dil,H,W,N', [(8, 16, 3, 1, 1, 1, 7, 9, 2), (16, 8, 5, 2, 2, 1, 11, 10, 1),
                                                             (32, 24, 1, 2, 0, 1, 5, 5, 3), (8, 8, 3, 1, 2, 2, 9, 8, 2),
                                                             (48, 24, 2, 1, 0, 1, 6, 4, 2), (8, 8, 3, 1, 1, 1, 1, 1, 1)])
def test_references_agree_with_int64_einsum(kind, cin, cout, k, stride, pad, dil, H, W, N):
    g = E.gen(cin, cout, k, H)
    K = cin * k * k
    x = E.operand(kind, (N, cin, H, W), K, g)
    w = E.operand(kind, (cout, cin, k, k), K, g)
    E.check_bound(K, x, w)
    want = E.conv_ref_int(x, w, stride, pad, dil)
    r64 = E.conv_ref(x, w, stride, pad, dil)
    r32 = E.conv_ref_f32(x, w, stride, pad, dil)
    assert r64.dtype == torch.float64 and torch.equal(r64.to(torch.int64), want) and torch.equal(r64, want.double())
    assert torch.equal(r32.double(), r64)
    assert torch.equal(E.cast(r64, torch.float32), r32)


@pytest.mark.parametrize('stride,pad,k,H,W', [(1, 1, 3, 6, 7), (2, 1, 3, 9, 10), (2, 0, 1, 7, 7), (2, 2, 5, 12, 11), (1, 0, 2, 5, 5)])
def test_gradient_references_agree_with_autograd_of_the_integer_conv(stride, pad, k, H, W):
    g = E.gen(stride, pad, k, H)
    cin, cout, N = 8, 16, 2
    x = E.wide((N, cin, H, W), g)
    w = E.wide((cout, cin, k, k), g)
    y = E.conv_ref(x, w, stride, pad)
    gy = E.wide(tuple(y.shape), g)
    xg = x.double().requires_grad_()
    wg = w.double().requires_grad_()
    torch.nn.functional.conv2d(xg, wg, None, stride, pad).backward(gy.double())
    assert torch.equal(E.dgrad_ref(gy, w, stride, pad, (H, W)), xg.grad)
    assert torch.equal(E.wgrad_ref(x, gy, k, k, stride, pad), wg.grad)
    assert torch.equal(E.wgrad_ref(-x.abs(), gy, k, k, stride, pad, x_abs=True), E.wgrad_ref(x.abs(), gy, k, k, stride, pad))
    assert torch.equal(xg.grad, xg.grad.round()) and torch.equal(wg.grad, wg.grad.round())


@pytest.mark.parametrize('K', [64, 1024, 2048, 4608, 9408])
def test_narrow_rule_keeps_outputs_bf16_exact(K):
    """K p_x p_w <= 1024 -> std <= 32; 4096 outputs per K stay within 256 (8 sigma), so each is a bf16-exact integer."""
    g = E.gen(K)
    p = E.narrow_p(K)
    assert K * p * p <= 1024 * 1.0000001 or p == 0.75 and K * p * p <= 1024
    x = E.narrow((64, K), K, g)
    w = E.narrow((64, K), K, g)
    assert set(torch.unique(x).tolist()) <= {-1.0, 0.0, 1.0} and (x == 0).any() and (x != 0).any()
    E.check_bound(K, x, w)
    ref = x.double() @ w.double().t()
    E.check_narrow(ref)
    assert ref.std().item() <= 32.0 * 1.1
    assert ref.abs().max().item() >= 8          # (the outputs are not trivially small either)
    assert torch.equal(E.cast(ref, torch.bfloat16).double(), ref)
    with pytest.raises(AssertionError):
        E.check_narrow(ref * 300)


def test_wide_outputs_exercise_the_bf16_rounding_and_its_ties():
    """512 -> 256 channels, 3x3 (K = 4608): the f32 conv equals the f64 one, the outputs run into the hundreds, a good share of
    them changes under the bf16 store and exact round-to-even ties (odd integers in 256..512) occur."""
    g = E.gen(4608)
    x = E.wide((1, 512, 10, 10), g)
    w = E.wide((256, 512, 3, 3), g)
    E.check_bound(4608, x, w, E.bias_ints(256, g), E.residual_ints((4,), g))
    r64 = E.conv_ref(x, w, 1, 1)
    assert torch.equal(E.conv_ref_f32(x, w, 1, 1).double(), r64)
    assert r64.abs().max().item() <= 9 * 4608 and r64.abs().max().item() > 512
    b = E.cast(r64, torch.bfloat16).double()
    assert 0.05 < (b != r64).double().mean().item() < 0.5
    a = r64.abs()
    assert int(((a > 256) & (a < 512) & (a % 2 == 1)).sum()) > 100
    trunc = (r64.float().view(torch.int32) & -65536).view(torch.float32).double()       # the store a truncating kernel would make
    assert (trunc != b).any()


def test_symbol_ties_are_met():
    """Medians that are multiples of 0.25 do produce exact .5 ties on integer outputs, so round-half-to-even is what the symbol cases
    of the GPU file pin (the operands of its 16 -> 40, 3x3 generic case)."""
    g = E.gen(16, 40, 3, 3, 7, 50, 3, 0, True)
    x, w = E.wide((3, 16, 7, 50), g), E.wide((40, 16, 3, 3), g)
    E.bias_ints(40, g)
    med = E.quarter_medians(40, g)
    d = E.conv_ref(x, w, 1, 1) - med.double().view(1, -1, 1, 1)
    ties = (d - torch.floor(d)) == 0.5
    assert int(ties.sum()) > 100
    r = torch.round(d[ties])
    assert torch.equal(r % 2, torch.zeros_like(r))          # torch.round is half-to-even, as rintf


def test_bound_and_integer_checks_refuse():
    g = E.gen(1)
    x, w = E.wide((4, 4), g), E.wide((4, 4), g)
    with pytest.raises(AssertionError):
        E.check_bound(1 << 22, x + 4.0 * (x == 0), w + 4.0 * (w == 0))
    with pytest.raises(AssertionError):
        E.check_bound(16, x * 0.5 + 0.25, w)
    with pytest.raises(AssertionError):
        E.check_bound(16, x + 257.0, w)          # 257 + small: not bf16 exact
    with pytest.raises(AssertionError):
        E.cast(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), torch.bfloat16)
    m = E.quarter_medians(32, g)
    assert torch.equal(m * 4, (m * 4).round()) and m.abs().max().item() <= 2


def test_assert_bits_equal_points_at_the_mismatch():
    ref = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).reshape(2, 3, 4, 8).to(torch.bfloat16)
    E.assert_bits_equal(ref.clone(), ref, 'same')
    got = ref.clone()
    got[1, 2, 1:3, 4:8] += 1
    with pytest.raises(AssertionError) as e:
        E.assert_bits_equal(got, ref, 'row')
    text = str(e.value)
    assert '8 of 192 elements differ' in text and 'first at (n, oh, ow, c) = (1, 2, 1, 4)' in text
    assert 'ONE output row' in text and 'ow in 1..2' in text and 'c//4 = 1' in text
    got = ref.clone()
    got[0, 0, 0, 0] = float('nan')
    with pytest.raises(AssertionError) as e:
        E.assert_bits_equal(got, ref, 'nan')
    assert '1 NaN' in str(e.value)
    with pytest.raises(AssertionError) as e:      # NCHW tensors are reported in (n, oh, ow, c) too
        E.assert_bits_equal(E.nchw(ref) + (torch.arange(8).view(1, 8, 1, 1) == 5), E.nchw(ref), 'channel', layout='nchw')
    assert 'c = 5' in str(e.value) and 'ONE' not in str(e.value)
    with pytest.raises(AssertionError):
        E.assert_bits_equal(ref.float(), ref, 'dtype')
    with pytest.raises(AssertionError) as e:
        E.assert_bits_equal(torch.zeros(3, 5), torch.ones(3, 5), '2-d')
    assert 'd1 in 0..4' in str(e.value)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32, torch.int32])
@pytest.mark.parametrize('shape', [(3, 5, 7, 8), (1,), (130, 33)])
def test_arena_view_is_contiguous_aligned_and_surrounded_by_fill(dtype, shape):
    t = torch.arange(int(torch.tensor(shape).prod())).reshape(shape).to(dtype)
    v = E.arena(t)
    assert v.is_contiguous() and v.shape == t.shape and v.dtype == dtype and torch.equal(v, t)
    assert v.data_ptr() % E.ALIGN == 0
    raw, off, nbytes, value = v._arena
    assert off >= E.GUARD_BYTES and raw.numel() - off - nbytes >= E.GUARD_BYTES and nbytes == t.numel() * t.element_size()
    assert v.data_ptr() == raw.data_ptr() + off
    lo, hi, pattern = E.bands(v)
    assert lo.numel() * v.element_size() >= E.GUARD_BYTES and hi.numel() * v.element_size() >= E.GUARD_BYTES
    assert E.bands_untouched(v)
    band_lo = raw[:off].view(dtype)
    band_hi = raw[off + nbytes:].view(dtype)
    if dtype.is_floating_point:
        assert torch.isnan(band_lo).all() and torch.isnan(band_hi).all()
    else:
        assert (band_lo == E.INT_SENTINEL[dtype]).all() and (band_hi == E.INT_SENTINEL[dtype]).all()
    E.assert_bands_untouched(v, 'fresh')
    v.view(-1)[0] = 1          # writes inside the view leave the bands alone
    assert E.bands_untouched(v)
    raw[off + nbytes + 6:off + nbytes + 8] = 0      # one element past the end
    assert not E.bands_untouched(v)
    with pytest.raises(AssertionError) as e:
        E.assert_bands_untouched(v, 'past the end')
    assert 'ABOVE' in str(e.value)
    o = E.arena_like(shape, dtype, 'cpu')
    assert E.bands_untouched(o) and (torch.isnan(o).all() if dtype.is_floating_point else (o == E.INT_SENTINEL[dtype]).all())
