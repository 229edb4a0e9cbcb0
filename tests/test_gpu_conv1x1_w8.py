"""-m gpu: the eight-wave 256-channel 1x1 kernel (conv1x1_w8.hip).

1. Bit equality with conv1x1_win_fwd on the same pack_conv_win weights (the kernel keeps that kernel's accumulation and epilogue
   order): ragged last tile, less than one tile, one to eight channel chunks, both strides, an odd map, the shortest and the longest
   K, and a launch with more units than CUs (static shares, joined K loops) repeated five times behind a different shape.
2. Exact integers (tests/exact_ints.py): operands in NaN arenas, the output in an arena whose bands stay untouched; no tolerance.
3. The `supported` predicates, and those of the kernels it takes layers from, unchanged.
4. A bs-2 HipHead with the policy '0' / '1' / 'all': outputs agree within the tolerance of the head's own test against torch, and with
   '1' the tags on the new kernel are exactly head._W8_TABLE, with 'all' every supported layer that is launched on its own.  (The tags
   come from a wrapper around hip.conv1x1_w8_fwd: hip.KernelTimer records a launch's tag, not its kernel; it supplies the set of tags
   launched one layer at a time.)
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import exact_ints as E  # noqa: E402

BF16 = torch.bfloat16
# (cin, cout, N, HW, stride, residual, relu)
SHAPES = [
    (1024, 256, 3, 14, 1, False, True),     # 588 px = two tiles + a ragged one, one channel chunk
    (512, 2048, 1, 7, 1, True, True),       # 49 px: less than one tile, eight chunks, residual
    (512, 1024, 2, 28, 2, False, False),    # stride 2 on an even map
    (256, 256, 1, 5, 2, False, True),       # odd map 5 -> 3, short K
    (128, 256, 2, 9, 1, False, False),      # one slab: the fewest loop trips
    (2048, 512, 5, 7, 1, False, True),      # longest K
    (512, 2048, 70, 14, 1, True, True),     # 62 tiles x 8 chunks = 496 units: more than one per CU
]
TABLE = [(1024, 256, 1), (1024, 512, 1), (512, 1024, 2), (1024, 2048, 2), (512, 2048, 1), (2048, 512, 1)]


@functools.lru_cache(maxsize=None)
def _random_case(cin, cout, N, HW, stride, res):
    """Operands on the host, made once per shape."""
    g = torch.Generator().manual_seed(cin * 7 + cout * 3 + N + HW + stride)
    x = torch.randn(N, HW, HW, cin, generator=g).to(BF16)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    OH = (HW - 1) // stride + 1
    r = torch.randn(N, OH, OH, cout, generator=g).to(BF16) if res else None
    return x, w, b, r


def _both(S, dev, cin, cout, N, HW, stride, res, relu):
    hip = S.hip
    x, w, b, r = _random_case(cin, cout, N, HW, stride, res)
    xd, wf, bd = x.to(dev), hip.pack_conv_win(w.to(dev)), b.to(dev)
    rd = r.to(dev) if r is not None else None
    want = hip.conv1x1_win_fwd(xd, wf, bd, stride=stride, residual=rd, relu=relu)
    return want, lambda: hip.conv1x1_w8_fwd(xd, wf, bd, stride=stride, residual=rd, relu=relu)


@pytest.mark.parametrize('cin,cout,N,HW,stride,res,relu', SHAPES[:-1])
def test_bits_equal_conv1x1_win(S, dev, cin, cout, N, HW, stride, res, relu):
    assert S.hip.conv1x1_w8_supported(cin, cout, 1, 1, stride, 0)
    want, run = _both(S, dev, cin, cout, N, HW, stride, res, relu)
    got = run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all())
    E.assert_bits_equal(got, want, 'conv1x1_w8 vs conv1x1_win {}->{} s{} N{} {}x{}'.format(cin, cout, stride, N, HW, HW))


def test_more_units_than_cus_repeats_bit_for_bit(S, dev):
    """496 units: every workgroup runs a share of them back to back.  Five launches behind a launch of a different shape."""
    _, other = _both(S, dev, *SHAPES[0])
    want, run = _both(S, dev, *SHAPES[-1])
    other()
    outs = [run() for _ in range(5)]
    torch.cuda.synchronize()
    for i, got in enumerate(outs):
        E.assert_bits_equal(got, want, 'conv1x1_w8, 496 units, launch {}'.format(i))


@pytest.mark.parametrize('kind', ['wide', 'narrow'])
@pytest.mark.parametrize('cin,cout,N,HW,stride,res,relu', SHAPES[:4])
def test_exact_integers(S, dev, kind, cin, cout, N, HW, stride, res, relu):
    hip = S.hip
    g = E.gen(cin, cout, N, HW, stride, kind == 'wide')
    x = E.operand(kind, (N, cin, HW, HW), cin, g)
    w = E.operand(kind, (cout, cin, 1, 1), cin, g)
    bias = E.bias_ints(cout, g)
    conv = E.conv_ref_int(x, w, stride, 0).double()
    if kind == 'narrow':
        E.check_narrow(conv)
    r = E.residual_ints(tuple(conv.shape), g) if res else None
    E.check_bound(cin, x, w, bias, r)
    ref = conv + bias.double().view(1, -1, 1, 1)
    if r is not None:
        ref = ref + r.double()
    if relu:
        ref = torch.relu(ref)
    xd = E.arena(E.nhwc(x).to(BF16), device=dev)
    wf = E.arena(hip.pack_conv_win(w.to(dev)), device=dev)
    bd = E.arena(bias, device=dev)
    rd = E.arena(E.nhwc(r), device=dev) if r is not None else None
    out = E.arena_like((N, conv.shape[2], conv.shape[3], cout), BF16, dev)
    got = hip.conv1x1_w8_fwd(xd, wf, bd, stride=stride, residual=rd, relu=relu, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    what = 'conv1x1_w8 {}->{} s{} N{} {}x{} res {} relu {} {}'.format(cin, cout, stride, N, HW, HW, res, relu, kind)
    E.assert_bits_equal(got, E.nhwc(E.cast(ref, BF16)), what)
    E.assert_bands_untouched(out, what)


def test_supported_predicates(S, dev):
    hip = S.hip
    for cin, cout, stride in TABLE:
        assert hip.conv1x1_w8_supported(cin, cout, 1, 1, stride, 0)
        assert bool(hip.lib().sc2_conv1x1_w8_supported(cin, cout, stride))
        assert not hip.conv1x1_w8_supported(cin, cout, 1, 1, 3, 0)
        assert not hip.conv1x1_w8_supported(cin + 64, cout, 1, 1, stride, 0)
        assert not hip.conv1x1_w8_supported(cin, cout + 128, 1, 1, stride, 0)
        assert not hip.conv1x1_w8_supported(cin, cout, 3, 3, stride, 1)
    assert not hip.conv1x1_w8_supported(64, 256, 1, 1, 1, 0) and not hip.conv1x1_w8_supported(128, 128, 1, 1, 1, 0)
    # the kernels it takes layers from answer what they answered (tests/test_gpu_kernels.py: test_conv1x1_kres, test_conv1x1_win)
    for cin, cout, stride in [(1024, 256, 1), (1024, 512, 1), (1024, 128, 1), (1024, 2048, 2), (2048, 512, 1), (2048, 64, 2), (2048, 1024, 1)]:
        assert bool(hip.lib().sc2_conv1x1_kres_supported(cin, cout, stride))
        assert hip.conv1x1_kres_supported(cin, cout, 1, 1, stride, 0) == (cin == 1024)
        assert not hip.conv1x1_kres_supported(512, cout, 1, 1, 1, 0)
        assert not hip.conv1x1_kres_supported(cin, cout, 1, 1, 3, 0)
    for cin, cout, stride in [(1024, 256, 1), (512, 2048, 1), (512, 1024, 2), (256, 128, 2), (128, 128, 1), (2048, 512, 1)]:
        assert hip.conv1x1_win_supported(cin, cout, 1, 1, stride, 0)
        assert not hip.conv1x1_win_supported(cin, cout, 1, 1, 3, 0)
        assert not hip.conv1x1_win_supported(cin + 64, cout, 1, 1, stride, 0)
        assert not hip.conv1x1_win_supported(cin, cout, 3, 3, stride, 1)


def test_head_policy(S, dev, monkeypatch):
    """A bs-2 HipHead on a 56 x 56 x 256 feature under conv1x1_w8 = '0', '1', 'all'.  Tolerance: that of the head against its torch
    reference (tests/test_gpu_bottleneck.py::test_hip_head_folded_bn: 0.05 * scale + 0.05)."""
    hip = S.hip
    from sc2bench_amd import head as head_mod
    torch.manual_seed(5)
    cfg = {'key': 'FPBasedResNetBottleneck', 'kwargs': {'num_bottleneck_channels': 24, 'num_target_channels': 256}}
    model = S.splittable_resnet(cfg, skips_avgpool=False, skips_fc=False, num_classes=1000)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
    model.eval().to(dev).set_compute_dtype('bf16')
    xb = torch.randn(2, 256, 56, 56).to(dev).to(BF16).contiguous(memory_format=torch.channels_last)
    on_w8 = []
    real = hip.conv1x1_w8_fwd

    def spy(x, w, b, **kw):
        on_w8.append((kw.get('tag'), x.shape[3], w.shape[1] * 16, kw.get('stride', 1)))
        return real(x, w, b, **kw)

    monkeypatch.setattr(hip, 'conv1x1_w8_fwd', spy)
    before = hip.host_policy.conv1x1_w8
    outs = {}
    try:
        for mode in ('0', '1', 'all'):
            hip.configure(conv1x1_w8=mode)
            del on_w8[:]
            with torch.no_grad(), hip.KernelTimer() as timer:
                outs[mode] = model.head(xb).float().cpu()
            launched = set(rec[0] for rec in timer.records)     # tags of the launches made one layer at a time
            if mode == '0':
                assert not on_w8
            elif mode == '1':
                assert sorted(set(t[1:] for t in on_w8)) == sorted(head_mod._W8_TABLE)
                tags = set(t[0] for t in on_w8)
                want = set()
                for c1, c2, c3, ds in model._hip_head.blocks:
                    for c in (c1, c2, c3, ds):
                        if c is not None and c.k == (1, 1) and (c.cin, c.cout, c.stride[0]) in head_mod._W8_TABLE:
                            want.add(c.tag)
                assert tags == want
            else:      # every supported layer that is launched on its own (layer2's pair launches carry their layers themselves)
                want = set(c.tag for blk in model._hip_head.blocks for c in blk if c is not None and c.w8_ok) & launched
                assert set(t[0] for t in on_w8) == want and len(want) >= 11
                for t in on_w8:
                    assert hip.conv1x1_w8_supported(t[1], t[2], 1, 1, t[3], 0)
    finally:
        hip.configure(conv1x1_w8=before)
    scale = outs['0'].abs().max().item()
    assert scale > 0
    for mode in ('1', 'all'):
        assert (outs[mode] - outs['0']).abs().max().item() <= 0.05 * scale + 0.05, mode
