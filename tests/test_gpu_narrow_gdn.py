"""-m gpu: the squared-form GDN of the bf16 transforms (entropy.GDN.forward_nhwc -> sc2_conv2d_fwd with SC2_AOP_SQUARE and
SC2_EPI_GDN2 / SC2_EPI_IGDN2) on NARROW layers, C <= 96: gamma travels zero-padded to the 128 packed rows of the kernel's tile.

Two checks per case.  (1) Bit for bit against the SAME layer embedded in a 128-channel one (gamma in the corner block, zero
elsewhere, beta 1 and x 0 on the added channels): the added products are exact zeros, so the first C channels must not differ.
(2) Against the float64 formula on the bf16-rounded gamma and the bf16 input, f32 output: the only roundings left are x^2 to bf16
on its way to the matrix cores (2^-9 relative on each term of a sum of non-negative terms, hence on the sum; half of it after
the square root) and f32 arithmetic, so 2^-9 |ref| bounds the error with room to spare."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CASES = [(32, 1, 5, 7), (40, 2, 3, 50), (96, 1, 9, 31), (8, 1, 1, 1)]     # C, N, H, W: 35 .. 300 pixels (more than one 128-pixel tile), one pixel


def _layer(S, C, inverse, seed):
    g = torch.Generator().manual_seed(seed)
    m = S.GDN(C, inverse=inverse)
    with torch.no_grad():
        m.gamma.copy_(m.gamma_reparam.init(0.1 * torch.eye(C) + 0.05 * torch.rand(C, C, generator=g)))
        m.beta.copy_(m.beta_reparam.init(0.5 + torch.rand(C, generator=g)))
    return m


@pytest.mark.parametrize('inverse', [False, True], ids=['gdn', 'igdn'])
@pytest.mark.parametrize('C,N,H,W', CASES, ids=lambda v: str(v))
def test_narrow_squared_gdn(S, dev, C, N, H, W, inverse):
    hip = S.hip
    m = _layer(S, C, inverse, 100 * C + H).to(dev)
    x = (3 * torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(C + W))).to(torch.bfloat16)
    xd = x.to(dev)
    beta, gamma_packed = m.effective()
    assert gamma_packed.shape[0] == 128 and not gamma_packed[C:].any()
    got_bf16 = m.forward_nhwc(xd)
    got_f32 = m.forward_nhwc(xd, out_format=hip.OUT_F32_NHWC)
    assert tuple(got_bf16.shape) == (N, H, W, C) and got_bf16.dtype == torch.bfloat16 and got_f32.dtype == torch.float32
    assert torch.equal(got_bf16, got_f32.to(torch.bfloat16))
    # (1) the same layer inside a 128-channel one
    wide = S.GDN(128, inverse=inverse)
    with torch.no_grad():       # the raw parameters copied into the corner: the reparametrisation is elementwise, so the block is m's
        wide.gamma.copy_(wide.gamma_reparam.init(torch.zeros(128, 128)))
        wide.beta.copy_(wide.beta_reparam.init(torch.ones(128)))
        wide.gamma[:C, :C] = m.gamma.detach().cpu()
        wide.beta[:C] = m.beta.detach().cpu()
    wide.to(dev)
    assert torch.equal(wide.effective()[1][:C, :C], gamma_packed[:C, :C]) and torch.equal(wide.effective()[0][:C], beta)
    xw = torch.zeros(N, H, W, 128, dtype=torch.bfloat16)
    xw[..., :C] = x
    for fmt, got in ((hip.OUT_BF16_NHWC, got_bf16), (hip.OUT_F32_NHWC, got_f32)):
        ref = wide.forward_nhwc(xw.to(dev), out_format=fmt)
        assert torch.equal(ref[..., :C].contiguous().view(torch.int16 if fmt == hip.OUT_BF16_NHWC else torch.int32),
                           got.view(torch.int16 if fmt == hip.OUT_BF16_NHWC else torch.int32))
    # (2) the float64 formula
    g64 = m.gamma_reparam(m.gamma).detach().to(torch.bfloat16).double().cpu()
    x64 = x.double()
    norm = torch.sqrt(torch.einsum('nhwk,ck->nhwc', x64 * x64, g64) + beta.double().cpu())
    want = x64 * norm if inverse else x64 / norm
    err = (got_f32.double().cpu() - want).abs()
    worst = (err / want.abs().clamp_min(1e-30))[want != 0].max().item() if (want != 0).any() else 0.0
    print('GDN C={} inverse={}: largest relative error {:.3g} (bound {:.3g})'.format(C, inverse, worst, 2.0 ** -9))
    assert bool((err <= 2.0 ** -9 * want.abs()).all())
