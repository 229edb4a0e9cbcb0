"""CPU: what the f32-grade codec modes of the hyperprior bottlenecks rest on that needs no device -- the stride-parity
decomposition of a transposed convolution (hip.deconv_parity_classes, shared by the bf16 and the precise forward of
HipConvTranspose2d), the restatement of the codec chain (tests/ref_split_hyper.py), and the mode switch itself."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_split_hyper as rh  # noqa: E402

# (kernel, stride, padding, output_padding)
GEOMETRIES = [(5, 2, 1, 0), (5, 2, 2, 1), (3, 1, 1, 0), (4, 2, 1, 0)]
INPUTS = [(1, 1), (2, 3), (5, 6)]


def scatter_classes(classes, x, stride, out_hw, conv=None):
    """The scattered sum of the per-class stride-1 correlations: x [N, Cin, H, W] -> [N, Cout, OH, OW] in x's dtype.
    Every output pixel must be written by exactly one class (the NaN pre-fill and the count say so)."""
    conv = conv or (lambda xp, sub: F.conv2d(xp, sub.to(xp.dtype)))
    (sh, sw), (OH, OW) = stride, out_hw
    out = torch.full((x.shape[0], classes[0].sub.shape[0], OH, OW), float('nan'), dtype=x.dtype)
    hits = torch.zeros(OH, OW, dtype=torch.int32)
    for c in classes:
        rows = (OH - c.off_h + sh - 1) // sh if OH > c.off_h else 0
        cols = (OW - c.off_w + sw - 1) // sw if OW > c.off_w else 0
        if rows == 0 or cols == 0:
            continue
        nkh, nkw = len(c.khs), len(c.kws)
        assert tuple(c.sub.shape[2:]) == (nkh, nkw)
        # zero padding (pad_h, pad_w) at the top / left, as much as the class's rows need at the bottom / right
        xp = F.pad(x, (c.pad_w, cols + nkw, c.pad_h, rows + nkh))
        out[:, :, c.off_h::sh, c.off_w::sw] = conv(xp, c.sub)[:, :, :rows, :cols]
        hits[c.off_h::sh, c.off_w::sw] += 1
    assert bool((hits == 1).all()), 'a pixel is written by {}..{} classes'.format(int(hits.min()), int(hits.max()))
    return out


@pytest.mark.parametrize('H,W', INPUTS)
@pytest.mark.parametrize('k,s,p,op', GEOMETRIES)
def test_parity_classes_equal_conv_transpose_on_integers(S, k, s, p, op, H, W):
    """Integer weights and inputs in f64: the scattered per-class correlations ARE F.conv_transpose2d, exactly."""
    g = torch.Generator().manual_seed(k * 1000 + s * 100 + p * 10 + H)
    cin, cout = 3, 5
    w = torch.randint(-3, 4, (cin, cout, k, k), generator=g).double()
    x = torch.randint(-3, 4, (2, cin, H, W), generator=g).double()
    ref = F.conv_transpose2d(x, w, None, s, p, op)
    classes = S.hip.deconv_parity_classes(w, (s, s), (p, p))
    assert len(classes) == s * s
    assert sorted((c.off_h, c.off_w) for c in classes) == [(a, b) for a in range(s) for b in range(s)]
    for c in classes:      # the taps of a class: every s-th, and together every tap once per axis
        assert c.khs == list(range(c.khs[0], k, s)) and c.kws == list(range(c.kws[0], k, s)) and c.pad_h >= 0 and c.pad_w >= 0
        assert torch.equal(c.sub, w.permute(1, 0, 2, 3)[:, :, c.khs][:, :, :, c.kws].flip(2, 3))
    got = scatter_classes(classes, x, (s, s), tuple(ref.shape[2:]))
    assert not torch.isnan(got).any()
    assert torch.equal(got, ref)


def test_parity_classes_two_strides_and_paddings(S):
    """stride (2, 1) with padding (1, 2): offsets, taps and paddings are per axis."""
    g = torch.Generator().manual_seed(7)
    w = torch.randint(-3, 4, (2, 3, 5, 4), generator=g).double()
    x = torch.randint(-3, 4, (1, 2, 4, 5), generator=g).double()
    ref = F.conv_transpose2d(x, w, None, (2, 1), (1, 2))
    got = scatter_classes(S.hip.deconv_parity_classes(w, (2, 1), (1, 2)), x, (2, 1), tuple(ref.shape[2:]))
    assert torch.equal(got, ref)


def test_parity_class_without_taps_raises(S):
    with pytest.raises(S.hip.Sc2Error, match='without taps'):
        S.hip.deconv_parity_classes(torch.zeros(4, 4, 1, 1), (2, 2), (0, 0))
    m = S.HipConvTranspose2d(8, 8, kernel_size=1, stride=2, padding=0, bias=False)
    with pytest.raises(S.hip.Sc2Error, match='without taps'):
        m._classes()


def test_bf16_path_packs_the_helper_sub_filters(S):
    """HipConvTranspose2d._classes (the bf16 path) is the helper's decomposition: same offsets, tap counts and paddings."""
    m = S.HipConvTranspose2d(16, 24, kernel_size=5, stride=2, padding=1, bias=False)
    want = [(c.off_h, c.off_w, len(c.khs), len(c.kws), c.pad_h, c.pad_w) for c in S.hip.deconv_parity_classes(m.weight, (2, 2), (1, 1))]
    assert [tuple(c[:6]) for c in m._classes()] == want
    assert want == [(0, 0, 2, 2, 1, 1), (0, 1, 2, 3, 1, 1), (1, 0, 3, 2, 1, 1), (1, 1, 3, 3, 1, 1)]


@pytest.mark.parametrize('ns', [2, 3])
def test_restatement_split_conv_transpose(S, ns):
    """The restatement's split transposed convolution: exact on bf16-exact integers (the low parts vanish), within the dropped
    products of F.conv_transpose2d on random floats (2^-16 / 2^-24 relative per operand pair), and equal -- summed in f64 -- to
    the per-class split correlations of the helper: the sum the device forms."""
    g = torch.Generator().manual_seed(ns)
    xi = torch.randint(-3, 4, (2, 4, 5, 6), generator=g).float()
    wi = torch.randint(-3, 4, (4, 6, 5, 5), generator=g).float()
    assert torch.equal(rh.split_conv_transpose(xi, wi, 2, 1, ns, torch.float64), F.conv_transpose2d(xi.double(), wi.double(), None, 2, 1))
    x = torch.randn(2, 4, 5, 6, generator=g)
    w = torch.randn(4, 6, 5, 5, generator=g) / 10
    ref = F.conv_transpose2d(x.double(), w.double(), None, 2, 1)
    got = rh.split_conv_transpose(x, w, 2, 1, ns, torch.float64)
    bound = {2: 3 * 2.0 ** -17, 3: 4 * 2.0 ** -25}[ns]      # the dropped part pairs: (1,1) .. resp. (1,2), (2,1), (2,2)
    assert (got - ref).abs().max().item() <= bound * (x.abs().double().sum(1).max() * w.abs().max()).item() * 25
    assert (got - ref).abs().max().item() > 0 or ns == 3
    import ref_split_encoder as rs
    per_class = scatter_classes(S.hip.deconv_parity_classes(w, (2, 2), (1, 1)), x, (2, 2), tuple(ref.shape[2:]),
                                conv=lambda xp, sub: rs.split_conv(xp, sub.float(), 1, 0, ns, torch.float64).float()).double()
    # (the same exact products, each class's in f64, rounded once to f32)
    assert (per_class - got).abs().max().item() <= 2.0 ** -23 * got.abs().max().item()


def test_restatement_chain_shapes(R):
    """chain() returns (z symbols, indexes, y symbols); in 'f32' arithmetic it is the oracle's encode path, integer for integer."""
    torch.manual_seed(0)
    bl = rh.shape_like_bench(R.MSHPBasedResNetBottleneck()).eval()
    bl.update()
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    z_sym, idx, y_sym = rh.chain(bl, x, 'f32')
    with torch.no_grad():
        y = bl.g_a(x)
        z = bl.h_a(y)
        z_hat = bl.entropy_bottleneck.quantize(z, 'dequantize', bl._get_means(z))
        sc, mu = bl.h_s(z_hat).chunk(2, 1)
        assert torch.equal(z_sym, bl.entropy_bottleneck.symbols(z).int())
        assert torch.equal(idx, bl.gaussian_conditional.build_indexes(sc).int())
        assert torch.equal(y_sym, bl.gaussian_conditional.quantize(y, 'symbols', mu).int())
    assert z_sym.dtype == idx.dtype == y_sym.dtype == torch.int32 and idx.shape == y_sym.shape == y.shape
    for mode in ('f64', 2, 3):
        got = rh.chain(bl, x, mode)
        assert [t.shape for t in got] == [z_sym.shape, idx.shape, y_sym.shape]
        assert (got[2] != y_sym).float().mean().item() < 1e-2
    assert rh.identical_images((z_sym, idx, y_sym), (z_sym, idx, y_sym)) == [True]


@pytest.mark.parametrize('name', ['SHPBasedResNetBottleneck', 'MSHPBasedResNetBottleneck'])
def test_mode_switch(S, name):
    m = S.get_layer(name)
    keys = list(m.state_dict().keys())
    assert m.encoder_precision == 'bf16' and m._precise_ns() is None
    for mode, ns in (('f32', 0), ('bf16x3', 2), ('bf16x6', 3), ('bf16', None)):
        assert m.set_encoder_precision(mode) is m and m.encoder_precision == mode and m._precise_ns() == ns
        assert m.set_compute_dtype(mode) is m
    fp = S.get_layer('FPBasedResNetBottleneck')
    with pytest.raises(ValueError) as e_fp:
        fp.set_encoder_precision('fp8')
    with pytest.raises(ValueError) as e_shp:
        m.set_encoder_precision('fp8')
    assert str(e_shp.value) == str(e_fp.value)
    assert m.encoder_precision == 'bf16'
    # the mode is no part of the state: keys unchanged, and a round trip through state_dict leaves it alone
    m.set_encoder_precision('bf16x6')
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert m.encoder_precision == 'bf16x6'
    other = S.get_layer(name)
    other.load_state_dict(sd)
    assert other.encoder_precision == 'bf16'
    assert 'decode' in type(m).set_encoder_precision.__doc__


def test_splittable_resnet_forwards_the_switch(S):
    cfg = {'key': 'MSHPBasedResNetBottleneck', 'kwargs': {'num_latent_channels': 16, 'num_bottleneck_channels': 24,
                                                           'num_target_channels': 256}}
    model = S.splittable_resnet(cfg, skips_avgpool=False, skips_fc=False, num_classes=10)
    assert model.set_encoder_precision('bf16x6') is model and model.bottleneck_layer.encoder_precision == 'bf16x6'
    with pytest.raises(ValueError):
        model.set_encoder_precision('fp8')


def test_precise_sequence_refuses_what_it_cannot_run(S):
    """No silent fall-back to bf16: a CPU input, another slope and a foreign module all raise Sc2Error."""
    from torch import nn
    x = torch.zeros(1, 4, 4, 16)
    seq = nn.Sequential(S.HipConv2d(16, 16, 3, 1, 1, bias=False))
    with pytest.raises(S.hip.Sc2Error):
        S.entropy.run_hip_sequence_precise(seq, x, 0)
    m = S.get_layer('SHPBasedResNetBottleneck').set_encoder_precision('f32')
    with pytest.raises(S.hip.Sc2Error):
        m.hyper_synthesis(torch.zeros(1, 4, 4, 16, dtype=torch.bfloat16))
