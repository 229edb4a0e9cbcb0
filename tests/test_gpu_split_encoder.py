"""-m gpu: the split-bf16 encoder modes (`set_encoder_precision('bf16x3' / 'bf16x6')`, csrc/conv_split.hip).

Every f32 operand is a sum of two / three bf16 parts and the kernel sums the part products with index sum <= 1 / <= 2 in f32 on
v_mfma_f32_16x16x32_bf16.  Each product is exact in f32, so against the restatement (tests/ref_split_encoder.py) summed in f64
only the f32 summation separates the two: the f32 mode's own per-launch tolerances hold (F32_TOL = 2e-6 * max|ref| for a
convolution, 4e-6 for a GDN1), and a missing or doubled cross term (2^-9 or 2^-17 relative) cannot hide in them.
Measured on an MI355X (each test prints its figures): one launch against the f64 sum of the same products 0.4e-7 - 2.8e-7 of max|ref|
(1.9e-7 / 2.6e-7 at K = 2 400; with one accumulation chain instead of chains of four k-steps: 1.09e-6 / 1.57e-6), 'bf16x6' against torch's
CPU f32 conv up to 6.0e-7; GDN1 0.8e-7 - 2.0e-7 (against the oracle's GDN1 up to 8.2e-7), fused conv + GDN1 up to 1.4e-6; symbols of 64
bench images: 'bf16x3' 5.0e-6 (restatement 5.4e-6, bound 1.58e-5), 45 images identical; 'bf16x6' 6.5e-7 (restatement 4.3e-7, bound
5.9e-6), 61 images identical; 'bf16' 3.2e-3."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, os.path.dirname(HERE))

import ref_split_encoder as rs  # noqa: E402

F32_TOL = 2e-6
GDN_TOL = 4e-6
MODES = {'bf16x3': 2, 'bf16x6': 3}


def _close(got, ref, tol, what=''):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print('{}: max abs err {:.3e} = {:.3e} * max|ref| (bound {:.1e})'.format(what, err, err / scale, tol))
    assert err <= tol * scale + 1e-30, '{}: max abs err {} vs scale {}'.format(what, err, scale)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('cin,cout,k,s,p,hw', [(3, 96, 5, 2, 2, (37, 50)), (96, 48, 5, 2, 2, (28, 31)), (48, 24, 2, 1, 0, (13, 9)),
                                               (24, 16, 5, 2, 1, (17, 17)), (8, 200, 3, 1, 1, (10, 12)), (4, 5, 1, 1, 0, (7, 5))])
def test_conv_split_vs_restatement(S, dev, mode, cin, cout, k, s, p, hw):
    """One launch against the f64 sum of the same exact products: what the bf16 MFMA's internal 32-term sum and the f32
    accumulation across k-steps cost."""
    ns = MODES[mode]
    g = torch.Generator().manual_seed(cin * 131 + cout)
    x = torch.randn(3, cin, hw[0], hw[1], generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g)
    ref = rs.split_conv(x, w, s, p, ns, acc=torch.float64)
    hip = S.hip
    xh = hip.nchw_f32_to_nhwc_f32(x.to(dev))
    wf = hip.pack_conv_split(w.to(dev), ns)
    y = hip.conv2d_split_fwd(xh, wf, cout, k, k, s, p, ns)
    tag = '{} {}->{} k{}'.format(mode, cin, cout, k)
    _close(y.permute(0, 3, 1, 2), ref, F32_TOL, tag + ' vs f64 sum of the split products')
    if ns == 3:
        _close(y.permute(0, 3, 1, 2), F.conv2d(x, w, None, s, p), F32_TOL, tag + ' vs the CPU f32 conv')
    y2 = hip.conv2d_split_fwd(xh, wf, cout, k, k, s, p, ns, out_format=hip.OUT_F32_NCHW)
    assert torch.equal(y2.cpu(), y.permute(0, 3, 1, 2).cpu())
    if cin == 3:      # the NCHW image given as it is: the same result
        y4 = hip.conv2d_split_fwd(x.to(dev).contiguous(), wf, cout, k, k, s, p, ns, x_is_nchw_rgb=True)
        assert torch.equal(y4.cpu(), y.cpu())
    yb = hip.conv2d_split_fwd(xh, wf, cout, k, k, s, p, ns, epilogue=hip.EPI_BIAS, ep_beta=b.to(dev), out_format=hip.OUT_F32_NCHW)
    _close(yb, ref + b.double().view(1, -1, 1, 1), F32_TOL, tag + ' + bias')
    if ns == 3:
        _close(yb, F.conv2d(x, w, b, s, p), F32_TOL, tag + ' + bias vs the CPU f32 conv')
    med = torch.linspace(-0.4, 0.4, cout)
    sym = hip.conv2d_split_fwd(xh, wf, cout, k, k, s, p, ns, out_format=hip.OUT_I32_NCHW_SYM, ep_beta=(med * 0.1).to(dev))
    want = torch.round(y2.cpu() * 1.0 - (med * 0.1).view(1, -1, 1, 1)).int()      # from the kernel's own f32 output: exact
    assert sym.dtype == torch.int32 and torch.equal(sym.cpu(), want)


def _gdn_pair(S, R, dev, C, inverse, seed):
    torch.manual_seed(seed)
    ref = R.GDN1(C, inverse=inverse)
    with torch.no_grad():
        ref.gamma.add_(0.02 * torch.rand_like(ref.gamma))
        ref.beta.add_(0.1 * torch.rand_like(ref.beta))
    g = S.GDN1(C, inverse=inverse)
    g.load_state_dict(ref.state_dict())
    g.to(dev)
    g._tag = 't'
    return ref, g


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('C,inverse', [(96, False), (48, False), (512, True), (20, False)])
def test_gdn1_split_vs_restatement_and_oracle(S, R, dev, mode, C, inverse):
    ns = MODES[mode]
    ref, g = _gdn_pair(S, R, dev, C, inverse, C)
    x = torch.randn(2, C, 9, 11)
    gamma, beta = S.FPBasedResNetBottleneck()._f32_pack(g, ns)
    hip = S.hip
    xh = hip.nchw_f32_to_nhwc_f32(x.to(dev))
    y = hip.conv2d_split_fwd(xh, gamma, C, 1, 1, 1, 0, ns, a_op=hip.AOP_ABS, epilogue=hip.EPI_IGDN if inverse else hip.EPI_GDN,
                             ep_x=xh, ep_beta=beta, out_format=hip.OUT_F32_NCHW)
    _close(y, rs.split_gdn(ref, x, ns, acc=torch.float64), GDN_TOL, '{} GDN1({}) vs the restatement'.format(mode, C))
    if ns == 3:
        with torch.no_grad():
            _close(y, ref(x), GDN_TOL, '{} GDN1({}) vs the oracle GDN1'.format(mode, C))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('cin,cout,k,s,p,inverse', [(3, 96, 5, 2, 2, False), (96, 48, 5, 2, 2, False), (8, 32, 3, 1, 1, True), (4, 20, 1, 1, 0, False)])
def test_conv_split_fused_gdn_equals_two_launches(S, R, dev, mode, cin, cout, k, s, p, inverse):
    ns = MODES[mode]
    hip = S.hip
    g = torch.Generator().manual_seed(cout)
    x = torch.randn(2, cin, 21, 18, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    ref, gdn = _gdn_pair(S, R, dev, cout, inverse, cout + 1)
    gamma, beta = S.FPBasedResNetBottleneck()._f32_pack(gdn, ns)
    xh = hip.nchw_f32_to_nhwc_f32(x.to(dev))
    wf = hip.pack_conv_split(w.to(dev), ns)
    t = hip.conv2d_split_fwd(xh, wf, cout, k, k, s, p, ns)
    two = hip.conv2d_split_fwd(t, gamma, cout, 1, 1, 1, 0, ns, a_op=hip.AOP_ABS, epilogue=hip.EPI_IGDN if inverse else hip.EPI_GDN,
                               ep_x=t, ep_beta=beta)
    one = hip.conv2d_split_fwd(xh, wf, cout, k, k, s, p, ns, epilogue=hip.EPI_FUSED_IGDN if inverse else hip.EPI_FUSED_GDN,
                               ep_x=gamma, ep_beta=beta)
    assert torch.isfinite(one).all() and torch.equal(one, two)
    want = rs.split_gdn(ref, rs.split_conv(x, w, s, p, ns, acc=torch.float64).float(), ns, acc=torch.float64)
    _close(one.permute(0, 3, 1, 2), want, GDN_TOL, '{} conv {}->{} + GDN1'.format(mode, cin, cout))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('cout', [64, 16, 80, 200])
def test_conv_split_fused_gdn_refused(S, dev, mode, cout):
    """A channel count the fused form does not cover is refused, never computed wrongly; so are other part counts."""
    ns = MODES[mode]
    hip = S.hip
    assert not hip.conv_split_fused_gdn_supported(cout)
    assert all(hip.conv_split_fused_gdn_supported(c) for c in (96, 48, 32, 20))
    g = torch.Generator().manual_seed(cout)
    x = torch.randn(1, 4, 9, 11, generator=g)
    w = torch.randn(cout, 4, 3, 3, generator=g) / 6.0
    gdn = S.GDN1(cout).to(dev)
    gdn._tag = 't'
    gamma, beta = S.FPBasedResNetBottleneck()._f32_pack(gdn, ns)
    xh = hip.nchw_f32_to_nhwc_f32(x.to(dev))
    wf = hip.pack_conv_split(w.to(dev), ns)
    with pytest.raises(hip.Sc2Error):
        hip.conv2d_split_fwd(xh, wf, cout, 3, 3, 1, 1, ns, epilogue=hip.EPI_FUSED_GDN, ep_x=gamma, ep_beta=beta)
    with pytest.raises(hip.Sc2Error):
        hip.pack_conv_split(w.to(dev), 4)
    d = hip.ConvDesc(N=1, H=9, W=11, Cin=4, Cout=cout, KH=3, KW=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, OH=9, OW=11,
                     a_op=hip.AOP_NONE, epilogue=hip.EPI_NONE, out_format=hip.OUT_F32_NHWC)
    y = torch.empty(1, 9, 11, cout, device=dev)
    assert hip.lib().sc2_conv2d_split_fwd(d, 4, xh.data_ptr(), wf.data_ptr(), y.data_ptr(), None, None, None, None) == -2


_BENCH = {}


def _bench_setup(dev):
    """bench.py's model, its oracle and 64 images of its batch; the oracle's symbols and the restatement's mismatch rates E(ns)."""
    if not _BENCH:
        import bench
        model = bench.build_model(dev)
        ref = bench.oracle_model(model.state_dict())
        x = bench.synthetic_batch(64, torch.device('cpu'))
        reb = ref.bottleneck_layer.entropy_bottleneck
        with torch.no_grad():
            ref_sym = torch.cat([reb.symbols(ref.bottleneck_layer.encoder(x[i:i + 16])) for i in range(0, 64, 16)])
            E = {}
            for ns in (2, 3):
                sym = torch.cat([reb.symbols(rs.split_encoder(ref.bottleneck_layer, x[i:i + 16], ns)) for i in range(0, 64, 16)])
                E[ns] = (sym != ref_sym).float().mean().item()
        _BENCH.update(bench=bench, model=model, ref=ref, x=x, ref_sym=ref_sym, E=E)
    return _BENCH


def test_split_encoder_symbols_vs_reference(S, R, dev):
    """64 bench images.  rate(mode) <= 2 E(ns) + 5e-6 with E(ns) the restatement's own rate; rate(bf16x6) <= rate(bf16x3) <
    rate(bf16) / 100; fused symbols == quantize(latent); identical symbols code to the oracle's bytes; >= 16 ('bf16x3') / >= 32
    ('bf16x6') of the 64 images have every symbol equal."""
    b = _bench_setup(dev)
    bench, model, ref, x, ref_sym, E = b['bench'], b['model'], b['ref'], b['x'], b['ref_sym'], b['E']
    bl = model.bottleneck_layer
    eb, reb = bl.entropy_bottleneck, ref.bottleneck_layer.entropy_bottleneck
    xd = x.to(dev)
    rate, sym_of = {}, {}
    try:
        with torch.no_grad():
            for mode in ('bf16', 'bf16x3', 'bf16x6'):
                model.set_encoder_precision(mode)
                sym, hw = model.stage_front(xd)
                sym_of[mode] = sym.cpu().view_as(ref_sym)
                rate[mode] = (sym_of[mode] != ref_sym).float().mean().item()
                if mode == 'bf16':
                    continue
                latent = bl.analysis(xd)
                assert torch.equal(sym_of[mode], reb.symbols(latent.cpu())), 'fused symbol output != quantize(latent)'
                buf, off, nb, st = eb.encode_symbols_device(sym, hw[0] * hw[1])
                assert int(st.max().item()) == 0
                exact = [i for i in range(64) if bool((sym_of[mode][i] == ref_sym[i]).all())]
                print('{}: mismatch rate {:.3e} (restatement E = {:.3e}, bound {:.3e}), {} of 64 images identical'.format(
                    mode, rate[mode], E[MODES[mode]], 2 * E[MODES[mode]] + 5e-6, len(exact)))
                if exact:
                    idx = torch.tensor(exact, device=dev)
                    streams = eb.unpack_strings(buf[idx], off[idx], nb[idx])
                    want = bench.oracle_streams(ref, ref_sym.reshape(64, -1)[exact], hw[0] * hw[1])
                    assert all(a == w for a, w in zip(streams, want)), 'same symbols, different bytes'
                assert rate[mode] <= 2 * E[MODES[mode]] + 5e-6
                assert len(exact) >= (16 if mode == 'bf16x3' else 32)
    finally:
        model.set_encoder_precision('bf16')
    print('bf16 mismatch rate {:.3e}'.format(rate['bf16']))
    assert rate['bf16x6'] <= rate['bf16x3'] < rate['bf16'] / 100


def test_mode_is_a_property_of_the_model(S, R, dev):
    """After the split modes 'bf16' and 'f32' give their earlier symbols again; batch sizes 1 and 3 agree with per-image runs; the
    batch-slicing path (a small slice limit) agrees with the unsliced one; 37 x 50 and 513 x 513 inputs match the restatement's
    symbols within the bound of the test above."""
    b = _bench_setup(dev)
    model, ref, x = b['model'], b['ref'], b['x']
    bl = model.bottleneck_layer
    eb, reb = bl.entropy_bottleneck, ref.bottleneck_layer.entropy_bottleneck
    xd = x[:5].to(dev)
    try:
        with torch.no_grad():
            before = {}
            for mode in ('bf16', 'f32'):
                model.set_encoder_precision(mode)
                before[mode] = bl.analysis(xd, symbols_for=eb).clone()
            for mode, ns in MODES.items():
                model.set_encoder_precision(mode)
                full = bl.analysis(xd[:3], symbols_for=eb).clone()
                for i in range(3):
                    assert torch.equal(bl.analysis(xd[i:i + 1], symbols_for=eb), full[i:i + 1]), (mode, i)
                # slices of two images (the limit is the size of two images' widest map), with and without the `out` buffer
                per_image = 4 * 96 * 112 * 112
                whole = bl.analysis(xd, symbols_for=eb).clone()
                sliced = bl._analysis_f32(xd, symbols_for=eb, ns=ns, slice_bytes=2 * per_image)
                assert torch.equal(sliced, whole), mode
                out = torch.empty(whole.numel(), dtype=torch.int32, device=dev)
                bl._analysis_f32(xd, symbols_for=eb, out=out, ns=ns, slice_bytes=2 * per_image)
                assert torch.equal(out.view_as(whole), whole), mode
                lat = bl._analysis_f32(xd, ns=ns, slice_bytes=2 * per_image)
                assert torch.equal(lat, bl.analysis(xd)), mode
                for hw in ((37, 50), (513, 513)):
                    xi = torch.randn(2, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(hw[0]))
                    got = bl.analysis(xi.to(dev), symbols_for=eb).cpu()
                    want = reb.symbols(rs.split_encoder(ref.bottleneck_layer, xi, ns))
                    r = (got.view_as(want) != want).float().mean().item()
                    print('{} {}x{}: {} symbols, mismatch vs the restatement {:.3e}'.format(mode, hw[0], hw[1], want.numel(), r))
                    assert r <= 2 * b['E'][ns] + 5e-6
            for mode in ('bf16', 'f32'):
                model.set_encoder_precision(mode)
                assert torch.equal(bl.analysis(xd, symbols_for=eb), before[mode]), mode
            with pytest.raises(ValueError):
                model.set_encoder_precision('fp8')
    finally:
        model.set_encoder_precision('bf16')


def test_split_pipeline_round_trip(S, R, dev):
    """stage_front -> stage_coder -> stage_back on 8 images in 'bf16x3': the decoded symbols are the encoder's, status 0."""
    b = _bench_setup(dev)
    model, x = b['model'], b['x']
    xd = x[:8].to(dev)
    try:
        with torch.no_grad():
            model.set_encoder_precision('bf16x3')
            sym, hw = model.stage_front(xd)
            dec, nb, st = model.stage_coder(sym, hw)
            assert int(st.max().item()) == 0 and int(nb.min().item()) > 0
            assert dec.dtype == torch.int32 and torch.equal(dec.view_as(sym), sym)
            out = model.stage_back(dec, hw)
            logits = out if torch.is_tensor(out) else list(out.values())[-1] if isinstance(out, dict) else out[-1]
            assert logits.shape[0] == 8 and torch.isfinite(logits.float()).all()
    finally:
        model.set_encoder_precision('bf16')
