"""-m gpu: what the precise kernels (csrc/conv_f32.hip, conv_split.hip; the shared frame csrc/conv_precise.h) gained for the
hyperprior transforms h_a / h_s, launch by launch: output scatter, two paddings, the ReLU / LeakyReLU epilogues, and on top of
them HipConvTranspose2d.forward_nhwc_precise (one launch per stride-parity class into one output).

Tolerance: F32_TOL = 2e-6 * max|ref| against the f64 sum of the same products, the per-convolution bound of
tests/test_gpu_split_encoder.py (K per class <= 9 * 16 = 144 here, shorter than any case that bound was set on).  Everything else
is bit for bit: activations against the same launch without them, 'f32' against one stride-1 launch on the zero-inserted input,
integer operands against the integer convolution."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import exact_ints as E  # noqa: E402
import ref_split_hyper as rh  # noqa: E402

F32_TOL = 2e-6
MODES = {'f32': 0, 'bf16x3': 2, 'bf16x6': 3}
KINDS = ['wide', 'narrow']
# (N, Cin, Cout, H, W): 1 x 1; odd sizes; two channel chunks' worth of tiles; classes of 225 / 210 / 210 / 196 pixels per image
# (around the 128-pixel workgroup tile and the 32-pixel wave tile); MSHP's second h_s layer; the non-vector channel path (Cout % 4)
SHAPES = [(1, 16, 16, 1, 1), (3, 16, 16, 2, 3), (2, 16, 24, 5, 6), (2, 16, 16, 14, 14), (1, 16, 24, 29, 27), (2, 8, 6, 4, 4)]


def _fwd(S, ns):
    hip = S.hip
    if ns == 0:
        return hip.pack_conv_f32, hip.conv2d_f32_fwd
    return (lambda w: hip.pack_conv_split(w, ns)), (lambda *a, **k: hip.conv2d_split_fwd(*a, ns=ns, **k))


def _deconv(S, dev, cin, cout, w=None, k=5, s=2, p=1):
    m = S.HipConvTranspose2d(cin, cout, kernel_size=k, stride=s, padding=p, bias=False)
    if w is not None:
        with torch.no_grad():
            m.weight.copy_(w)
    return m.to(dev)


def _ref64(x, w, ns, s=2, p=1):
    """f64 sum of the products the mode forms: all of them ('f32'), or the part pairs with i + j <= ns - 1."""
    if ns == 0:
        return F.conv_transpose2d(x.double(), w.double(), None, s, p)
    return rh.split_conv_transpose(x, w, s, p, ns, acc=torch.float64)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('N,cin,cout,H,W', SHAPES)
def test_precise_deconv_vs_restatement(S, dev, mode, N, cin, cout, H, W):
    ns = MODES[mode]
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + H)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cin, cout, 5, 5, generator=g) / (cin * 9) ** 0.5
    m = _deconv(S, dev, cin, cout, w)
    ref = _ref64(x, w, ns)
    OH, OW = ref.shape[2:]
    assert (OH, OW) == (2 * H + 1, 2 * W + 1)
    xd = S.hip.nchw_f32_to_nhwc_f32(x.to(dev))
    scale = ref.abs().max().item()
    for act, epi, fn in ((None, S.hip.EPI_NONE, lambda t: t), ('relu', S.hip.EPI_BIAS_RELU, F.relu),
                         ('leaky', S.hip.EPI_BIAS_LEAKY_RELU, lambda t: F.leaky_relu(t, 0.01))):
        out = torch.full((N, OH, OW, cout), float('nan'), dtype=torch.float32, device=dev)
        with torch.no_grad():
            got = m.forward_nhwc_precise(xd, ns, epi, out=out)
        assert got is out
        got = got.cpu()
        assert not torch.isnan(got).any(), '{} pixels left unwritten'.format(int(torch.isnan(got).any(-1).sum()))
        err = (got.permute(0, 3, 1, 2).double() - fn(ref)).abs().max().item()
        print('{} {} act {}: max abs err {:.3e} = {:.3e} * max|ref| (bound {:.1e})'.format(mode, (N, cin, cout, H, W), act, err, err / scale, F32_TOL))
        assert err <= F32_TOL * scale
    with torch.no_grad():     # without `out=`: the same tensor from the forward's own allocation
        assert torch.equal(m.forward_nhwc_precise(xd, ns, S.hip.EPI_BIAS_LEAKY_RELU).cpu(), got)


@pytest.mark.parametrize('mode', list(MODES))
def test_activation_epilogues_bit_for_bit(S, dev, mode):
    """EPI_BIAS_RELU / EPI_BIAS_LEAKY_RELU = torch's CPU activation of the SAME launch's plain output (+ bias in f32), with and
    without a bias vector: h_a's first conv (24 -> 16, k5 s2 p1, 17 x 17, |x| on load), NHWC and NCHW, and a transposed conv."""
    hip, ns = S.hip, MODES[mode]
    pack, fwd = _fwd(S, ns)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 24, 17, 17, generator=g)
    w = torch.randn(16, 24, 5, 5, generator=g) / 24.0
    b = torch.randn(16, generator=g) * 0.3
    xd, wf, bd = hip.nchw_f32_to_nhwc_f32(x.to(dev)), pack(w.to(dev)), b.to(dev)
    acts = ((hip.EPI_BIAS_RELU, F.relu), (hip.EPI_BIAS_LEAKY_RELU, lambda t: F.leaky_relu(t, 0.01)))
    for fmt, shape_b in ((hip.OUT_F32_NHWC, (1, 1, 1, -1)), (hip.OUT_F32_NCHW, (1, -1, 1, 1))):
        plain = fwd(xd, wf, 16, 5, 5, 2, 1, a_op=hip.AOP_ABS, out_format=fmt).cpu()
        assert (plain < 0).any() and (plain > 0).any()
        for epi, fn in acts:
            got = fwd(xd, wf, 16, 5, 5, 2, 1, a_op=hip.AOP_ABS, epilogue=epi, out_format=fmt).cpu()
            assert torch.equal(got, fn(plain)), 'epilogue {} without bias'.format(epi)
            got = fwd(xd, wf, 16, 5, 5, 2, 1, a_op=hip.AOP_ABS, epilogue=epi, ep_beta=bd, out_format=fmt).cpu()
            assert torch.equal(got, fn(plain + b.view(shape_b))), 'epilogue {} with bias'.format(epi)
    # the transposed convolution: the activation in each class's epilogue; a module bias rides with it
    m = S.HipConvTranspose2d(16, 24, kernel_size=5, stride=2, padding=1, bias=True)
    with torch.no_grad():
        m.bias.copy_(torch.randn(24, generator=g) * 0.3)
    m.to(dev)
    xt = hip.nchw_f32_to_nhwc_f32(torch.randn(2, 16, 6, 5, generator=g).to(dev))
    with torch.no_grad():
        plain = m.forward_nhwc_precise(xt, ns).cpu()          # (EPI_BIAS: the bias is in)
        for epi, fn in acts:
            assert torch.equal(m.forward_nhwc_precise(xt, ns, epi).cpu(), fn(plain))


@pytest.mark.parametrize('N,cin,cout,H,W', [s for s in SHAPES if s[1] % 16 == 0])
def test_f32_classes_equal_one_stride1_launch(S, dev, N, cin, cout, H, W):
    """'f32': the class launches equal ONE stride-1 launch of conv2d_f32_fwd on the zero-inserted input with the full flipped
    filter (padding k - 1 - p = 3), bit for bit (torch.equal ignores the sign of zero).  Why, and for which shapes: the kernel walks
    K in steps of 16 and inside a step issues four MFMAs, MFMA j taking k = 16 s + 4 q + j of the four lane quarters q -- an fma
    chain ordered by (step, j, q), not by k.  With Cin % 16 == 0 a tap fills whole steps, so a class's taps and the full filter's
    (the class's taps with all-zero taps between them) run the same chain per tap, and a product with an exact zero leaves the
    chain unchanged.  With Cin = 8 a step holds TWO taps and a class pairs other taps in a step than the full filter does: the
    same products in another order, equal only within rounding.  That shape is held to F32_TOL and to the integer results above
    and below instead."""
    hip = S.hip
    g = torch.Generator().manual_seed(cin + cout + H)
    x = torch.randn(N, cin, H, W, generator=g)
    m = _deconv(S, dev, cin, cout)
    xz = torch.zeros(N, cin, 2 * H - 1, 2 * W - 1)
    xz[:, :, ::2, ::2] = x
    w_full = m.weight.detach().permute(1, 0, 2, 3).flip(2, 3).contiguous()
    want = hip.conv2d_f32_fwd(hip.nchw_f32_to_nhwc_f32(xz.to(dev)), hip.pack_conv_f32(w_full), cout, 5, 5, 1, 3)
    with torch.no_grad():
        got = m.forward_nhwc_precise(hip.nchw_f32_to_nhwc_f32(x.to(dev)), 0)
    assert got.shape == want.shape == (N, 2 * H + 1, 2 * W + 1, cout)
    assert torch.equal(got.cpu(), want.cpu())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N,cin,cout,H,W', [(2, 16, 24, 7, 6), (1, 16, 16, 14, 14), (2, 8, 6, 4, 4)])
def test_precise_deconv_equals_the_integer_deconv(S, dev, kind, N, cin, cout, H, W):
    """Integer operands in NaN arenas: all three modes equal conv_transpose2d bit for bit; the scatter output sits in an arena
    whose bands stay untouched."""
    K = cin * 9
    g = E.gen(N, cin, cout, H, W, kind == 'wide')
    x = E.operand(kind, (N, cin, H, W), K, g)
    w = E.operand(kind, (cin, cout, 5, 5), K, g)
    E.check_bound(K, x, w)
    ref = F.conv_transpose2d(x.double(), w.double(), None, 2, 1)
    if kind == 'narrow':
        E.check_narrow(ref)
    want = E.nhwc(E.cast(ref, torch.float32))
    m = _deconv(S, dev, cin, cout, w)
    xd = E.arena(E.nhwc(x), device=dev)
    for mode, ns in MODES.items():
        for epi, fn in ((S.hip.EPI_NONE, lambda t: t), (S.hip.EPI_BIAS_RELU, F.relu)):      # (relu of integers: integers)
            out = E.arena_like(tuple(want.shape), torch.float32, dev)
            with torch.no_grad():
                got = m.forward_nhwc_precise(xd, ns, epi, out=out)
            torch.cuda.synchronize()
            tag = '{} deconv {} epi {} {}'.format(mode, (N, cin, cout, H, W), epi, kind)
            E.assert_bits_equal(got, fn(want), tag)
            E.assert_bands_untouched(out, tag)


@pytest.mark.parametrize('kind', KINDS)
def test_scatter_drops_pixels_outside_the_output(S, dev, kind):
    """out_H / out_W smaller than the classes reach: the pixels outside are dropped, the rest is the cropped result, the bands
    of the output arena stay intact."""
    hip = S.hip
    N, cin, cout, H, W = 2, 16, 24, 6, 7
    g = E.gen(N, cin, cout, H, W, kind == 'wide', 3)
    x = E.operand(kind, (N, cin, H, W), cin * 9, g)
    w = E.operand(kind, (cin, cout, 5, 5), cin * 9, g)
    ref = F.conv_transpose2d(x.double(), w.double(), None, 2, 1)
    OH, OW = ref.shape[2:]
    crop = E.nhwc(E.cast(ref, torch.float32))[:, :OH - 3, :OW - 2].contiguous()
    xd = E.arena(E.nhwc(x), device=dev)
    for mode, ns in MODES.items():
        pack, fwd = _fwd(S, ns)
        out = E.arena_like(tuple(crop.shape), torch.float32, dev)
        for c in hip.deconv_parity_classes(w.to(dev), (2, 2), (1, 1)):
            rows, cols = (OH - c.off_h + 1) // 2, (OW - c.off_w + 1) // 2      # as for the FULL output: some land outside `out`
            got = fwd(xd, E.arena(pack(c.sub), device=dev), cout, len(c.khs), len(c.kws), 1, (c.pad_h, c.pad_w),
                      scatter=(rows, cols, out, 2, 2, c.off_h, c.off_w))
            assert got is out
        torch.cuda.synchronize()
        E.assert_bits_equal(out, crop, '{} cropped scatter {}'.format(mode, kind))
        E.assert_bands_untouched(out, '{} cropped scatter {}'.format(mode, kind))


@pytest.mark.parametrize('kind', KINDS)
def test_hs_tail_conv_equals_the_integer_conv(S, dev, kind):
    """h_s's last layer (24 -> 48, k5 p0; MSHP) on integer operands, all three modes, with the activation epilogues."""
    hip = S.hip
    N, cin, cout, H, W = 2, 24, 48, 13, 11
    g = E.gen(N, cin, cout, H, W, kind == 'wide', 5)
    x = E.operand(kind, (N, cin, H, W), cin * 25, g)
    w = E.operand(kind, (cout, cin, 5, 5), cin * 25, g)
    bias = E.bias_ints(cout, g)
    E.check_bound(cin * 25, x, w, bias)
    ref = E.conv_ref(x, w, 1, 0)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd, bd = E.arena(E.nhwc(x), device=dev), E.arena(bias, device=dev)
    for mode, ns in MODES.items():
        pack, fwd = _fwd(S, ns)
        wf = E.arena(pack(w.to(dev)), device=dev)
        got = fwd(xd, wf, cout, 5, 5, 1, (0, 0), out_format=hip.OUT_F32_NCHW)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, E.cast(ref, torch.float32), mode + ' tail conv ' + kind, layout='nchw')
        got = fwd(xd, wf, cout, 5, 5, 1, (0, 0), epilogue=hip.EPI_BIAS_RELU, ep_beta=bd, out_format=hip.OUT_F32_NCHW)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, E.cast(F.relu(ref + bias.double().view(1, -1, 1, 1)), torch.float32), mode + ' tail conv + bias + relu ' + kind,
                            layout='nchw')


@pytest.mark.parametrize('kind', KINDS)
def test_two_paddings_equal_the_integer_conv(S, dev, kind):
    """pad_h != pad_w on a dense (unscattered) launch, stride 2: both axes take their own padding."""
    N, cin, cout, H, W = 2, 8, 20, 9, 10
    g = E.gen(N, cin, cout, H, W, kind == 'wide', 7)
    x = E.operand(kind, (N, cin, H, W), cin * 15, g)
    w = E.operand(kind, (cout, cin, 3, 5), cin * 15, g)
    ref = E.conv_ref(x, w, 2, (0, 2))
    xd = E.arena(E.nhwc(x), device=dev)
    for mode, ns in MODES.items():
        pack, fwd = _fwd(S, ns)
        got = fwd(xd, E.arena(pack(w.to(dev)), device=dev), cout, 3, 5, 2, (0, 2))
        torch.cuda.synchronize()
        E.assert_bits_equal(got, E.nhwc(E.cast(ref, torch.float32)), '{} pad (0, 2) {}'.format(mode, kind))


@pytest.mark.parametrize('mode', list(MODES))
def test_refusals(S, dev, mode):
    """What the widened contract still refuses: each with SC2_ERR_UNSUPPORTED (-2), raised as Sc2Error."""
    hip, ns = S.hip, MODES[mode]
    pack, fwd = _fwd(S, ns)
    x = torch.zeros(1, 4, 5, 16, device=dev)
    w = torch.zeros(32, 16, 2, 2, device=dev)
    wf = pack(w)
    out = torch.zeros(1, 9, 11, 32, device=dev)
    sc = (5, 6, out, 2, 2, 0, 0)
    beta = torch.ones(32, device=dev)
    unsupported = pytest.raises(hip.Sc2Error, match=r'code -2')
    with unsupported:      # scatter + fused GDN
        fwd(x, wf, 32, 2, 2, 1, (1, 1), epilogue=hip.EPI_FUSED_GDN, ep_x=pack(torch.eye(32, device=dev).view(32, 32, 1, 1)), ep_beta=beta, scatter=sc)
    with unsupported:      # scatter + the separate GDN epilogue
        fwd(x, wf, 32, 2, 2, 1, (1, 1), epilogue=hip.EPI_GDN, ep_x=torch.zeros(1, 5, 6, 32, device=dev), ep_beta=beta, scatter=sc)
    with unsupported:      # scatter + symbol output
        fwd(x, wf, 32, 2, 2, 1, (1, 1), out_format=hip.OUT_I32_NCHW_SYM, ep_beta=beta, scatter=sc)
    with unsupported:      # scatter + f32 NCHW
        fwd(x, wf, 32, 2, 2, 1, (1, 1), out_format=hip.OUT_F32_NCHW, scatter=sc)
    with unsupported:      # stride_h != stride_w
        fwd(x, wf, 32, 2, 2, (2, 1), (0, 0))
    with unsupported:      # an epilogue the precise kernels do not have
        fwd(x, wf, 32, 2, 2, 1, (0, 0), epilogue=hip.EPI_BIAS_ADD_RELU, ep_beta=beta)
    assert float(out.abs().max()) == 0.0      # nothing was launched
    # Cout > 48 scatters too (the 96-channel instantiations kept their registers): no refusal to test there
    w96 = torch.randint(-2, 3, (96, 16, 2, 2)).float()
    x96 = torch.randint(-2, 3, (1, 16, 4, 5)).float()
    out96 = torch.full((1, 9, 11, 96), float('nan'), device=dev)
    fwd(E.nhwc(x96).to(dev), pack(w96.to(dev)), 96, 2, 2, 1, (1, 1), scatter=(5, 6, out96, 2, 2, 0, 0))
    want = E.nhwc(E.cast(E.conv_ref(x96, w96, 1, 1), torch.float32))
    assert torch.equal(out96[:, ::2, ::2].cpu(), want) and bool(torch.isnan(out96[:, 1::2]).all()) and bool(torch.isnan(out96[:, :, 1::2]).all())
