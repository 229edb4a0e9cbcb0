"""GPU: the kernels of the CR+BQ baseline (csrc/bq.hip) against the written-down contract (tests/ref_bq.py).

The quantizer and the f32 dequantizer are held to the bit: min / max are exact in any order and every other step is a single
IEEE f32 operation.  The bf16 outputs are held to one bf16 ulp of the float64 formula (the kernels round an f32 result to bf16
once: half an ulp, plus the f32 roundings in front of it, which the `slack` argument of `_within_bf16_ulp` bounds per case)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_bq as rb  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [2, 255, 256, 257, 4099, 2 * 12 * 9 * 9, 2 ** 20 + 3]


def _bits(t):
    return t.detach().cpu().reshape(-1).view(torch.int32).tolist()


def _within_bf16_ulp(got, want64, slack=None):
    """|got - want| <= 1 bf16 ulp of want (8 significant bits: 2^(exponent - 7)) + slack"""
    want64 = want64.double()
    mag = want64.abs().clamp_min(2.0 ** -126)
    ulp = torch.pow(2.0, torch.floor(torch.log2(mag)) - 7)
    tol = ulp if slack is None else ulp + slack
    err = (got.double().cpu() - want64).abs()
    bad = err > tol
    assert not bool(bad.any()), 'max err / tol {:.3f} at {} of {} elements'.format(float((err / tol).max()), int(bad.sum()), bad.numel())


def _check_quantize(S, dev, x, name):
    want = rb.quantize(x)
    q, scale, zp, status = S.hip.bq_quantize(x.to(dev))
    assert status.tolist() == [0], name
    assert q.dtype == torch.uint8 and q.shape == x.shape
    assert zp.tolist() == [want.zero_point], name
    assert _bits(scale) == _bits(want.scale), name
    assert torch.equal(q.cpu(), want.tensor), '{}: {} codes differ'.format(name, int((q.cpu() != want.tensor).sum()))
    return q, scale, zp


@pytest.mark.parametrize('n', SIZES)
def test_quantize_bit_exact(S, dev, n):
    sets = rb.edge_sets(n)
    for name, (x, zp, scale) in sets.items():        # on the CPU first: each set does what it is meant to do
        want = rb.quantize(x)
        assert zp is None or want.zero_point == zp, name
        assert scale is None or float(want.scale) == scale, name
    ties = rb.quantize(sets['ties'][0])
    if n >= 8:
        assert ties.tensor[1:5].tolist() == [6, 6, 8, 8]
    assert sets['extremes_first_last'][0].argmin() == 0 and sets['extremes_first_last'][0].argmax() == n - 1
    assert sets['extremes_last_first'][0].argmax() == 0 and sets['extremes_last_first'][0].argmin() == n - 1
    for name, (x, _, _) in sets.items():
        q, scale, zp = _check_quantize(S, dev, x, '{}[{}]'.format(name, n))
        back = S.hip.bq_dequantize(q, scale, zp)
        assert _bits(back) == _bits(rb.dequantize(rb.quantize(x))), name


def test_quantize_unaligned_start_and_shapes(S, dev):
    base = 3.0 * torch.randn(4100, generator=torch.Generator().manual_seed(5))
    view = base.to(dev)[1:]                 # contiguous, but 4 bytes off a 16-byte boundary: the scalar-load form
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    want = rb.quantize(base[1:].clone())
    q, scale, zp, status = S.hip.bq_quantize(view)
    assert status.tolist() == [0] and zp.tolist() == [want.zero_point] and _bits(scale) == _bits(want.scale)
    assert torch.equal(q.cpu(), want.tensor)
    x4 = 2.0 * torch.randn(2, 12, 9, 9, generator=torch.Generator().manual_seed(6)) + 1.0
    got = S.quantize_tensor(x4.to(dev))
    want = rb.quantize(x4)
    assert isinstance(got, S.QuantizedTensor) and got.tensor.is_cuda and got.tensor.shape == x4.shape
    assert got.scale.dim() == 0 and got.scale.is_cuda and isinstance(got.zero_point, int)
    assert torch.equal(got.tensor.cpu(), want.tensor) and _bits(got.scale) == _bits(want.scale) and got.zero_point == want.zero_point
    assert _bits(S.dequantize_tensor(got)) == _bits(rb.dequantize(want))


@pytest.mark.parametrize('n', [7, 256, 4099])
def test_quantize_status(S, dev, n):
    zeros = torch.zeros(n)
    nan = torch.randn(n, generator=torch.Generator().manual_seed(n))
    nan[n // 2] = float('nan')
    for name, bad in (('zeros', zeros), ('nan', nan)):
        with pytest.raises(ValueError):
            rb.quantize(bad)
        _, _, _, status = S.hip.bq_quantize(bad.to(dev))
        assert status.tolist() == [1], name
        with pytest.raises(ValueError):
            S.SimpleQuantizer(8)(bad.to(dev))
    # one bad image fails a per-sample batch, and only its status is set
    batch = torch.stack([torch.arange(n, dtype=torch.float32), zeros, nan]).to(dev)
    assert S.hip.bq_quantize(batch, per_sample=True)[3].tolist() == [0, 1, 1]
    with pytest.raises(ValueError):
        S.SimpleQuantizer(8, per_sample=True)(batch)


@pytest.mark.parametrize('shape', [(3, 12, 9, 9), (3, 1, 9, 9), (3, 4099)])
def test_quantize_per_sample(S, dev, shape):
    g = torch.Generator().manual_seed(len(shape))
    spread = torch.tensor([0.05, 1.0, 40.0]).reshape([3] + [1] * (len(shape) - 1))
    shift = torch.tensor([0.0, -3.0, 9.0]).reshape([3] + [1] * (len(shape) - 1))
    x = torch.randn(shape, generator=g) * spread + shift
    got = S.SimpleQuantizer(8, per_sample=True)(x.to(dev))
    assert got.scale.shape == (3,) and got.zero_point.shape == (3,) and got.tensor.shape == x.shape
    back = S.SimpleDequantizer(8)(got)
    zps = set()
    for i, want in enumerate(rb.quantize_per_sample(x)):
        alone = S.quantize_tensor(x[i].to(dev))
        assert torch.equal(got.tensor[i].cpu(), want.tensor) and torch.equal(alone.tensor.cpu(), want.tensor)
        assert _bits(got.scale[i]) == _bits(want.scale) == _bits(alone.scale)
        assert int(got.zero_point[i]) == want.zero_point == alone.zero_point
        assert _bits(back[i]) == _bits(rb.dequantize(want))
        zps.add(want.zero_point)
    assert len(zps) == 3          # the three images really have different ranges


def test_dequantize_f32_bit_exact(S, dev):
    codes = torch.arange(256, dtype=torch.uint8)
    for n in (256, 259):          # 259: three trailing codes behind the 4-code groups
        q = codes.repeat(2)[:n]
        for zp in (0, 64, 255):
            for scale in (1.0, 0.0085, 3.7e-5):
                s = torch.tensor(scale, dtype=torch.float32)
                want = s * (q.float() - zp)
                got = S.hip.bq_dequantize(q.to(dev), s.to(dev), zp)
                assert got.dtype == torch.float32 and _bits(got) == _bits(want), (n, zp, scale)
    # per image: three scales and zero points at once
    q3 = torch.stack([codes, codes.flip(0), codes.roll(7)])
    s3 = torch.tensor([1.0, 0.0085, 3.7e-5])
    z3 = torch.tensor([0, 64, 255], dtype=torch.int32)
    got = S.hip.bq_dequantize(q3.to(dev), s3.to(dev), z3.to(dev))
    want = s3.reshape(3, 1) * (q3.float() - z3.reshape(3, 1).float())
    assert _bits(got) == _bits(want)


@pytest.mark.parametrize('channels', [1, 3, 12])
@pytest.mark.parametrize('hw', [(9, 9), (10, 8)])
def test_dequantize_nhwc_affine_relu(S, dev, channels, hw):
    g = torch.Generator().manual_seed(channels * 100 + hw[0])
    q = torch.randint(0, 256, (2, channels) + hw, generator=g, dtype=torch.uint8)
    scale, zp = torch.tensor(0.0213, dtype=torch.float32), 97
    a = (0.5 + torch.rand(channels, generator=g)) * torch.where(torch.arange(channels) % 2 == 0, 1.0, -1.0)
    if channels > 1:
        assert bool((a > 0).any()) and bool((a < 0).any())
    b = 0.4 * torch.randn(channels, generator=g)
    cpad = (channels + 7) // 8 * 8
    v64 = scale.double() * (q.double() - zp)
    want = torch.relu(a.double().reshape(1, -1, 1, 1) * v64 + b.double().reshape(1, -1, 1, 1)).permute(0, 2, 3, 1)
    # f32 roundings in front of the bf16 one: v = scale * (q - zp) (2^-24 |v|, scaled by |a|) and the fma's own (2^-24 of the result)
    slack = 2.0 ** -23 * ((a.double().reshape(1, -1, 1, 1) * v64).abs().permute(0, 2, 3, 1) + want.abs())
    got = S.hip.bq_dequantize(q.to(dev), scale.to(dev), zp, out_format=S.hip.OUT_BF16_NHWC, affine=(a.to(dev), b.to(dev)), relu=True)
    assert got.dtype == torch.bfloat16 and got.shape == (2,) + hw + (cpad,) and got.is_contiguous()
    _within_bf16_ulp(got[..., :channels].float(), want, slack)
    assert int((got[..., channels:].view(torch.int16) != 0).sum()) == 0            # padding channels: exact zeros
    # plain form (bottleneck_idx 9): the f32 product rounded to bf16 once, per image scales
    s2, z2 = torch.tensor([0.0213, 1.5]), torch.tensor([97, 3], dtype=torch.int32)
    plain = S.hip.bq_dequantize(q.to(dev), s2.to(dev), z2.to(dev), out_format=S.hip.OUT_BF16_NHWC, cpad=16)
    want_plain = (s2.reshape(2, 1, 1, 1) * (q.float() - z2.reshape(2, 1, 1, 1).float())).to(torch.bfloat16).permute(0, 2, 3, 1)
    assert plain.shape == (2,) + hw + (16,)
    assert torch.equal(plain[..., :channels].cpu().view(torch.int16), want_plain.contiguous().view(torch.int16))
    assert int((plain[..., channels:].view(torch.int16) != 0).sum()) == 0


@pytest.mark.parametrize('hw', [(8, 8), (7, 9), (16, 16)])
@pytest.mark.parametrize('channels', [8, 64])
def test_maxpool_affine_relu(S, dev, hw, channels):
    g = torch.Generator().manual_seed(hw[0] * 64 + channels)
    x = torch.randn((2, channels) + hw, generator=g).to(torch.bfloat16)
    one, zero = torch.ones(channels, device=dev), torch.zeros(channels, device=dev)

    def run(inp, a, b):
        return S.hip.maxpool_affine_relu_nhwc(inp.permute(0, 2, 3, 1).contiguous().to(dev), a, b, 3, 2, 1).permute(0, 3, 1, 2).float().cpu()

    # the max itself, bit for bit: identity affine, ReLU defeated by an all-positive input
    pos = x.abs() + torch.tensor(0.125, dtype=torch.bfloat16)
    assert bool((pos > 0).all())
    want = F.max_pool2d(pos.float(), 3, 2, 1)
    got = run(pos, one, zero)
    assert got.shape == want.shape and torch.equal(got, want)
    # the affine follows the max: scales of both signs, and an all-negative input (the -inf padding of the borders must not win)
    a = (0.5 + torch.rand(channels, generator=g)) * torch.where(torch.rand(channels, generator=g) < 0.4, -1.0, 1.0)
    assert bool((a < 0).any()) and bool((a > 0).any())
    b = 0.5 * torch.randn(channels, generator=g)
    for inp in (x, -pos):
        m = F.max_pool2d(inp.float(), 3, 2, 1).double()
        want = torch.relu(a.double().reshape(1, -1, 1, 1) * m + b.double().reshape(1, -1, 1, 1))
        _within_bf16_ulp(run(inp, a.to(dev), b.to(dev)), want, 2.0 ** -23 * want.abs())


@pytest.mark.parametrize('hw', [(9, 9), (3, 2)])
@pytest.mark.parametrize('channels', [8, 512])
def test_avgpool2d(S, dev, hw, channels):
    g = torch.Generator().manual_seed(hw[0] + channels)
    x = torch.randn((2, channels) + hw, generator=g).to(torch.bfloat16)
    got = S.hip.avgpool2d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(dev), 2, 1)
    assert got.shape == (2, hw[0] - 1, hw[1] - 1, channels) and got.dtype == torch.bfloat16
    want = F.avg_pool2d(x.double(), 2, 1)
    # three f32 additions in front of the bf16 rounding: each at most 2^-24 of a partial sum, itself at most the sum of magnitudes
    slack = 3 * 2.0 ** -24 * F.avg_pool2d(x.double().abs(), 2, 1) * 4
    _within_bf16_ulp(got.permute(0, 3, 1, 2).float(), want, slack)
