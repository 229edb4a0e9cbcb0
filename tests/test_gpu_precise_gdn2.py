"""-m gpu: the squared-form GDN of the precise kernels (SC2_EPI_GDN2 / SC2_EPI_IGDN2 in csrc/conv_precise.h, the one epilogue of
csrc/conv_f32.hip and csrc/conv_split.hip), launch by launch, for ns = 0 ('f32'), 2 ('bf16x3') and 3 ('bf16x6').

Zero tolerance on integers: x in {-3..3}, gamma in {0, 1, 2}, beta integers >= 1, so norm = gamma x^2 + beta is an exact integer in
every mode (all parts are bf16-exact) and the output must equal the CPU's correctly rounded x * (1 / sqrt(norm)) resp.
x * sqrt(norm) bit for bit -- which pins the rounding of the device's sqrt and division (tests/test_input_modes_cpu.py shows the CPU
reference is correctly rounded on these values).  Operands sit in NaN arenas (tests/exact_ints.py).

Random f32 data: |device - oracle| <= delta = max(4e-6, 3 e_R) max|ref|, the oracle being compressai's GDN in torch's f32 ops and
e_R the error of the mode's restatement (tests/ref_split_input.py) against it.

Refusals are read from the returned status of the C entry points; the output buffer shows that nothing was launched."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import exact_ints as E  # noqa: E402
import ref_split_input as ri  # noqa: E402

MODES = {'f32': 0, 'bf16x3': 2, 'bf16x6': 3}
RESTATED = {0: 'f64', 2: 2, 3: 3}
FLOOR = 4e-6
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -2


def _fwd(S, ns):
    hip = S.hip
    if ns == 0:
        return hip.pack_conv_f32, hip.conv2d_f32_fwd
    return (lambda w: hip.pack_conv_split(w, ns)), (lambda *a, **k: hip.conv2d_split_fwd(*a, ns=ns, **k))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('pixels', ri.GDN2_PIXELS)
@pytest.mark.parametrize('C', ri.GDN2_CHANNELS)
def test_gdn2_integers_bit_for_bit(S, dev, C, pixels, mode):
    hip, ns = S.hip, MODES[mode]
    pack, fwd = _fwd(S, ns)
    x, gamma, beta, norm = ri.gdn2_int_case(C, pixels)
    E.check_bound(C, x * x, gamma, beta)
    xd = E.arena(E.nhwc(x), device=dev)
    gd = E.arena(pack(gamma.view(C, C, 1, 1).to(dev)), device=dev)
    bd = E.arena(beta, device=dev)
    for inverse, epi in ((False, hip.EPI_GDN2), (True, hip.EPI_IGDN2)):
        want = ri.gdn2_int_expected(x, norm, inverse)
        for fmt, layout in ((hip.OUT_F32_NHWC, 'nhwc'), (hip.OUT_F32_NCHW, 'nchw')):
            got = fwd(xd, gd, C, 1, 1, 1, 0, a_op=hip.AOP_SQUARE, epilogue=epi, ep_x=xd, ep_beta=bd, out_format=fmt)
            what = '{} C {} pixels {} {} {}'.format(mode, C, pixels, 'IGDN2' if inverse else 'GDN2', layout)
            E.assert_bits_equal(got, E.nhwc(want) if layout == 'nhwc' else want, what, layout=layout)
    for t, name in ((xd, 'x'), (gd, 'gamma'), (bd, 'beta')):
        E.assert_bands_untouched(t, name)


_PAIRS = {}


def _gdn_pair(S, dev, C, inverse):
    """(device GDN, oracle GDN) with gamma = 0.1 I + 0.02 rand and beta = 1 + rand."""
    from oracle import cpu_ref_input
    key = (C, inverse)
    if key not in _PAIRS:
        g = torch.Generator().manual_seed(C + int(inverse))
        ref = cpu_ref_input.GDN(C, inverse=inverse)
        with torch.no_grad():
            ref.gamma.copy_(ref.gamma_reparam.init(0.1 * torch.eye(C) + 0.02 * torch.rand(C, C, generator=g)))
            ref.beta.copy_(ref.beta_reparam.init(1.0 + torch.rand(C, generator=g)))
        m = S.GDN(C, inverse=inverse)
        m.load_state_dict(ref.state_dict())
        _PAIRS[key] = (m.to(dev), ref)
    return _PAIRS[key]


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('C,pixels', [(12, (2, 5, 7)), (100, (2, 5, 7)), (128, (3, 9, 11)), (192, (2, 5, 7))])
def test_gdn2_random_vs_restatement(S, dev, C, pixels, inverse, mode):
    hip, ns = S.hip, MODES[mode]
    m, ref = _gdn_pair(S, dev, C, inverse)
    N, H, W = pixels
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(C * 7 + H)) * 3.0
    with torch.no_grad():
        oracle = ref(x)
        rest = ri._ops(RESTATED[ns], torch.float32)[2](ref, x)
        xd = hip.nchw_f32_to_nhwc_f32(x.to(dev))
        got = m.forward_nhwc_precise(xd, ns)
        got_nchw = m.forward_nhwc_precise(xd, ns, out_format=hip.OUT_F32_NCHW)
    scale = oracle.abs().max().item()
    e_r = (rest.double() - oracle.double()).abs().max().item() / scale
    e_d = (got.cpu().permute(0, 3, 1, 2).double() - oracle.double()).abs().max().item() / scale
    delta = max(FLOOR, 3 * e_r)
    print('{} C {} {}: restatement error {:.2e}, device error {:.2e} of max|ref| {:.3g} (delta {:.2e})'.format(
        mode, C, 'IGDN2' if inverse else 'GDN2', e_r, e_d, scale, delta))
    assert e_d <= delta
    assert torch.equal(got_nchw.cpu(), got.cpu().permute(0, 3, 1, 2))      # the two formats hold the same values
    # the packing is cached per parameter version, and follows the parameters
    packed = m._precise_cache[ns][0]
    with torch.no_grad():
        assert torch.equal(m.forward_nhwc_precise(xd, ns), got) and m._precise_cache[ns][0] is packed


@pytest.mark.parametrize('mode', list(MODES))
def test_gdn2_refusals(S, dev, mode):
    """GDN2 / IGDN2 with output scatter (SC2_ERR_UNSUPPORTED), as symbols, without ep_x, without ep_beta (SC2_ERR_INVALID_ARG): read
    from the status of the C entry point; the NaN-filled output is untouched (no launch)."""
    hip, ns = S.hip, MODES[mode]
    pack, _ = _fwd(S, ns)
    C, N, H, W = 16, 1, 4, 4
    x = torch.ones(N, H, W, C, device=dev)
    gamma = pack(torch.eye(C, device=dev).view(C, C, 1, 1))
    beta = torch.ones(C, device=dev)
    y = torch.full((N, 2 * H, 2 * W, C), float('nan'), device=dev)
    L = hip.lib()

    def call(epi, fmt=hip.OUT_F32_NHWC, scatter=False, ep_x=x, ep_beta=beta):
        sc = dict(out_H=2 * H, out_W=2 * W, out_stride_h=2, out_stride_w=2, out_off_h=0, out_off_w=0) if scatter else {}
        d = hip.ConvDesc(N=N, H=H, W=W, Cin=C, Cout=C, KH=1, KW=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, OH=H, OW=W,
                         a_op=hip.AOP_SQUARE, epilogue=epi, out_format=fmt, **sc)
        p = hip._ptr
        if ns == 0:
            return L.sc2_conv2d_f32_fwd(ctypes.byref(d), p(x), p(gamma), p(y), p(ep_x), p(ep_beta), hip._stream())
        return L.sc2_conv2d_split_fwd(ctypes.byref(d), ns, p(x), p(gamma), p(y), p(ep_x), None, p(ep_beta), hip._stream())

    for epi in (hip.EPI_GDN2, hip.EPI_IGDN2):
        assert call(epi, scatter=True) == ERR_UNSUPPORTED
        assert 'scatter' in hip.last_error()
        assert call(epi, fmt=hip.OUT_I32_NCHW_SYM) == ERR_INVALID_ARG
        assert call(epi, ep_x=None) == ERR_INVALID_ARG
        assert call(epi, ep_beta=None) == ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
    assert call(hip.EPI_GDN2) == 0        # the same descriptor without the faults runs
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y.view(-1)[:N * H * W * C]).any())
