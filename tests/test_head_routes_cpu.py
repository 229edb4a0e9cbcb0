"""Which launch every layer of the task head takes, pinned without a GPU.

`head._Conv` routes a folded conv + norm layer to one of seven kernels by the layer's shape, the dispatch policy and the call's
epilogue.  This test replaces the launchers of `hip` with stubs that record what they were asked and return an empty CPU tensor of
the right shape, then runs

  * the forward of a ResNet-50 `HipHead` (layer1 .. fc) on a 2 x 56 x 56 x 64 map,
  * forward + backward of `FrozenStack` layer2 on 2 x 56 x 56 x 256 and of layer3 on 2 x 28 x 28 x 512

under twelve policy settings (each applied before the networks are built; the switches that are read per call once more on networks
built under the default), plus a few single cases under the default policy, and compares the launch sequences with
tests/golden/head_routes.json.  Only the launchers and `hip._dev` are faked: the library loads without a device, its `*_supported`
predicates answer and the packers run on CPU tensors.

Beside the sequence, every launch's weight and bias must equal the matching packer applied to that layer's `w_folded` / `b`
(pack_conv_win: w8, win1, win3; pack_weight_fragments: stream, kres, both operands of the pair; pack_conv_weight: the tile kernel),
so the fixture holds shapes and flags only, no float hashes.

`python tests/test_head_routes_cpu.py --write` rewrites the fixture from the code as it stands: {'records': the distinct launch
records, 'cases': {case: indices into records}}.
"""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'head_routes.json')
BF16 = torch.bfloat16

# policy settings applied BEFORE the networks are built
SETTINGS = collections.OrderedDict([
    ('default', {}),
    ('w8=0', {'conv1x1_w8': '0'}),
    ('w8=all', {'conv1x1_w8': 'all'}),
    ('win1=0', {'conv1x1_win': '0'}),
    ('win1=all', {'conv1x1_win': 'all'}),
    ('stream=0', {'conv_stream': False}),
    ('kres=0', {'conv_kres': 0}),
    ('kres=2,w8=0,win1=0', {'conv_kres': 2, 'conv1x1_w8': '0', 'conv1x1_win': '0'}),
    ('win=0', {'conv_win': False}),
    ('win_s2=0', {'conv_win_s2': False}),
    ('pair=0', {'conv1x1_pair': False}),
    ('mask_fused=0', {'relu_mask_fused': False}),
])
# the switches read at every call, applied AFTER building under the default
LATE = ('w8=0', 'w8=all', 'win=0', 'win_s2=0', 'mask_fused=0')


def _shape(t):
    return 'x'.join(str(int(v)) for v in t.shape)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(int(a) for a in v)


class Recorder(object):
    """The stubs.  `convs`: tag -> head._Conv of every layer that may launch, for the weight / bias check."""

    def __init__(self, hip, monkeypatch):
        self.hip, self.log, self.convs, self._want = hip, [], {}, {}
        monkeypatch.setattr(hip, '_dev', lambda t, name: t)
        for name in ('conv1x1_w8_fwd', 'conv1x1_win_fwd', 'conv1x1_stream_fwd', 'conv1x1_kres_fwd', 'conv3x3_win_fwd', 'conv2d_fwd',
                     'conv1x1_pair_fwd', 'relu_bwd', 'avgpool_nhwc', 'fc_fwd'):
            monkeypatch.setattr(hip, name, getattr(self, name))

    def register(self, *convs):
        for c in convs:
            if c is not None:
                assert self.convs.get(c.tag, c) is c, c.tag
                self.convs[c.tag] = c

    def _check(self, tag, layout, w, b):
        """w, b are what `layout`'s packer makes of the layer's folded weight and its bias"""
        c, hip = self.convs[tag], self.hip
        want = self._want.get((tag, layout))
        if want is None:
            w2d = c.w_folded.reshape(c.w_folded.shape[0], -1)
            want = self._want[(tag, layout)] = {'win': lambda: hip.pack_conv_win(c.w_folded),
                                                'frag': lambda: hip.pack_weight_fragments(w2d),
                                                'tile': lambda: hip.pack_conv_weight(c.w_folded, c.k_order)}[layout]()
        assert w.dtype == BF16 and w.shape == want.shape and torch.equal(w, want), (tag, layout)
        assert b is None or (b.dtype == torch.float32 and torch.equal(b, c.b)), (tag, layout)

    def _one(self, name, layout, cout, x, w, b, stride=1, residual=None, relu=False, tag=None, mask=None):
        self._check(tag, layout, w, b)
        self.log.append('{} {} {} {} s{} relu{:d} res{:d} mask{:d}'.format(name, tag, _shape(x), _shape(w), int(stride), bool(relu),
                                                                         residual is not None, mask is not None))
        N, H, W, _ = x.shape
        return N, H, W, cout

    def _out1x1(self, N, H, W, cout, stride):
        return torch.empty((N, (H - 1) // stride + 1, (W - 1) // stride + 1, cout), dtype=BF16)

    def conv1x1_w8_fwd(self, x, w, b, stride=1, residual=None, relu=False, tag=None, out=None):
        assert out is None
        return self._out1x1(*self._one('w8', 'win', w.shape[1] * 16, x, w, b, stride, residual, relu, tag), stride=stride)

    def conv1x1_win_fwd(self, x, w, b, stride=1, residual=None, relu=False, tag=None, mask=None):
        return self._out1x1(*self._one('win1', 'win', w.shape[1] * 16, x, w, b, stride, residual, relu, tag, mask), stride=stride)

    def conv1x1_stream_fwd(self, x, w, b, stride=1, residual=None, relu=False, tag=None, mask=None):
        return self._out1x1(*self._one('stream', 'frag', w.shape[0] * 16, x, w, b, stride, residual, relu, tag, mask), stride=stride)

    def conv1x1_kres_fwd(self, x, w, b, stride=1, relu=False, tag=None):
        return self._out1x1(*self._one('kres', 'frag', w.shape[0] * 16, x, w, b, stride, None, relu, tag), stride=stride)

    def conv3x3_win_fwd(self, x, w, b, relu=False, tag=None, stride=1, mask=None):
        N, H, W, cout = self._one('win3', 'win', w.shape[1] * 16, x, w, b, stride, None, relu, tag, mask)
        return torch.empty((N, H // 2, W // 2, cout) if stride == 2 else (N, H, W, cout), dtype=BF16)

    def conv2d_fwd(self, x, w, cout, kh, kw, stride, pad, a_op=0, epilogue=0, out_format=0, ep_x=None, ep_beta=None, out=None,
                   tag=None, scatter=None, k_order=0, dilation=1):
        hip = self.hip
        assert a_op == hip.AOP_NONE and out_format == hip.OUT_BF16_NHWC
        if tag in self.convs:      # (not the sub-filter launches of hip.conv2d_dgrad, tag 'dgrad')
            self._check(tag, 'tile', w, ep_beta)
        (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(pad), _pair(dilation)
        self.log.append('conv2d {} {} {} k{}x{} s{}x{} p{}x{} d{}x{} epi{} epx{:d} ko{} out{:d} scatter{}'.format(
            tag, _shape(x), _shape(w), kh, kw, sh, sw, ph, pw, dh, dw, epilogue, ep_x is not None, k_order, out is not None,
            '-' if scatter is None else 'x'.join(str(int(v)) for v in scatter[:2] + scatter[3:])))
        if scatter is not None:
            return scatter[2]
        if out is not None:
            return out
        N, H, W, _ = x.shape
        return torch.empty((N, (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1, cout), dtype=BF16)

    def conv1x1_pair_fwd(self, o, w3, b3, identity, w1, b1, tag=None):
        t3, t1 = tag.split('+')
        self._check(t3, 'frag', w3, b3)
        self._check(t1, 'frag', w1, b1)
        self.log.append('pair {} {} {} {}'.format(tag, _shape(o), _shape(w3), _shape(w1)))
        N, H, W, _ = o.shape
        assert tuple(identity.shape) == (N, H, W, w3.shape[0] * 16)
        return torch.empty((N, H, W, w3.shape[0] * 16), dtype=BF16), torch.empty((N, H, W, w1.shape[0] * 16), dtype=BF16)

    def relu_bwd(self, g, out, add=None):
        assert g.shape == out.shape and (add is None or add.shape == g.shape)
        self.log.append('relu_bwd {} add{:d}'.format(_shape(g), add is not None))
        return torch.empty_like(g)

    def avgpool_nhwc(self, x, want_f32=True, want_bf16=False):
        self.log.append('avgpool {}'.format(_shape(x)))
        N, C = x.shape[0], x.shape[3]
        return (torch.empty((N, C), dtype=torch.float32) if want_f32 else None, torch.empty((N, C), dtype=BF16) if want_bf16 else None)

    def fc_fwd(self, a, w, bias, tag=None):
        self.log.append('fc {} {} {}'.format(tag, _shape(a), _shape(w)))
        return torch.empty((a.shape[0], w.shape[0] * 16), dtype=torch.float32)

    def take(self):
        log, self.log = self.log, []
        return log


class Policy(object):
    """`with Policy(hip, conv_stream=False): ...` -- puts every touched field back."""

    def __init__(self, hip, **kw):
        self.hip, self.kw = hip, kw

    def __enter__(self):
        self.before = {k: getattr(self.hip.host_policy, k) for k in self.kw}
        self.hip.configure(**self.kw)

    def __exit__(self, *exc):
        self.hip.configure(**self.before)
        return False


def _model():
    from sc2bench_amd.resnet import resnet50
    torch.manual_seed(11)
    model = resnet50()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


class Nets(object):
    """The head and the two frozen stacks of one model, built under the policy in force, their layers registered with `rec`."""

    def __init__(self, rec, model):
        from sc2bench_amd.frozen import FrozenStack
        from sc2bench_amd.head import HipHead
        self.rec = rec
        rec.convs.clear()
        rec._want.clear()
        self.head = HipHead([(i + 1, getattr(model, 'layer{}'.format(i + 1))) for i in range(4)], model.fc)
        self.stacks = [(FrozenStack(n, getattr(model, n)), shape) for n, shape in (('layer2', (2, 56, 56, 256)), ('layer3', (2, 28, 28, 512)))]
        for blk in self.head.blocks:
            rec.register(*blk)
        for stack, _ in self.stacks:
            for blk, dg in zip(stack.blocks, stack._dg()):
                rec.register(*blk)
                rec.register(*[c for d in dg if d is not None for c in (d.as_conv, d.as_dense)])

    def run(self, key, cases):
        rec = self.rec
        self.head.forward(torch.empty((2, 56, 56, 64), dtype=BF16))
        cases[key + ' head'] = rec.take()
        for stack, shape in self.stacks:
            out, saved = stack.forward(torch.empty(shape, dtype=BF16), save=True)
            stack.backward(torch.empty_like(out), saved)
            cases['{} {}'.format(key, stack.name)] = rec.take()


def record_cases(hip, monkeypatch):
    """-> ({case: [launch record]}, the default-policy Nets)"""
    from sc2bench_amd import head as H
    rec = Recorder(hip, monkeypatch)
    model = _model()
    cases = collections.OrderedDict()
    for key, kw in SETTINGS.items():
        with Policy(hip, **kw):
            Nets(rec, model).run(key, cases)
    nets = Nets(rec, model)                   # built under the default ...
    for key in LATE:                          # ... the per-call switches flipped behind it
        with Policy(hip, **SETTINGS[key]):
            nets.run('late ' + key, cases)
    # a map size no window-plane 3x3 layer takes
    nets.head.forward(torch.empty((1, 40, 40, 64), dtype=BF16))
    cases['default head 40x40'] = rec.take()
    # dilated 3x3 layers: the descriptor's dilation (256 channels), the four phase grids (64 channels); a 7x7 stride-2 stem
    g = torch.Generator().manual_seed(12)
    for tag, cout, cin, k, stride, pad, dil, hw in (('dil256', 256, 256, 3, 1, 2, 2, 28), ('dil64', 64, 64, 3, 1, 2, 2, 28),
                                                    ('stem', 64, 8, 7, 2, 3, 1, 64)):
        w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        bn = torch.nn.BatchNorm2d(cout).eval()
        c = H._Conv(H.ConvSpec(w, (stride, stride), (pad, pad), (dil, dil)), bn, tag)
        rec.register(c)
        y = c(torch.empty((1, hw, hw, cin), dtype=BF16), hip.EPI_BIAS_RELU)
        assert tuple(y.shape) == (1, hw // stride, hw // stride, cout)
        cases['default ' + tag] = rec.take()
    # the two layers the decoder's last launch can take along
    tail = H.HipHead([(i, getattr(model, 'layer{}'.format(i))) for i in (2, 3, 4)], model.fc)
    spec = tail.tail_spec()
    c1, _, _, ds = tail.blocks[0]
    assert spec[0] is c1.w2d and spec[1] is c1.b and spec[2] is ds.w2d and spec[3] is ds.b
    assert torch.equal(c1.w2d, c1.w_folded.reshape(128, 256).to(BF16)) and torch.equal(ds.w2d, ds.w_folded.reshape(512, 256).to(BF16))
    cases['default tail_spec'] = ['tail_spec {} {} {} {}'.format(*[_shape(t) for t in spec])]
    return cases, nets


def _counts(log):
    return dict(collections.Counter(r.split(' ', 1)[0] for r in log))


def _encode(cases):
    records = sorted(set(r for log in cases.values() for r in log))
    index = {r: i for i, r in enumerate(records)}
    return {'records': records, 'cases': {k: [index[r] for r in log] for k, log in cases.items()}}


@pytest.fixture(scope='module')
def routes():
    import sc2bench_amd
    hip = sc2bench_amd.hip
    hip.lib()
    mp = pytest.MonkeyPatch()
    before = {k: getattr(hip.host_policy, k) for kw in SETTINGS.values() for k in kw}
    try:
        cases, nets = record_cases(hip, mp)
    finally:
        mp.undo()
    assert before == {k: getattr(hip.host_policy, k) for k in before}
    return cases, nets


def test_harness_counts(routes):
    """The launch counts of the default policy, as they were measured when the routing was pinned."""
    cases, _ = routes
    head = _counts(cases['default head'])
    assert head == {'win3': 13, 'stream': 12, 'w8': 11, 'conv2d': 6, 'pair': 4, 'win1': 2, 'avgpool': 1, 'fc': 1}
    both = collections.Counter(_counts(cases['default layer2'])) + collections.Counter(_counts(cases['default layer3']))
    assert dict(both) == {'stream': 24, 'win3': 18, 'relu_bwd': 10, 'conv2d': 8, 'kres': 7, 'win1': 7, 'w8': 6}

    def relu_bwds(key):
        return sum(_counts(cases['{} {}'.format(key, n)]).get('relu_bwd', 0) for n in ('layer2', 'layer3'))

    assert relu_bwds('mask_fused=0') == 30 and relu_bwds('late mask_fused=0') == 30 and relu_bwds('stream=0') == 18
    assert _counts(cases['default head 40x40'])['conv2d'] == 19
    assert _counts(cases['default dil256']) == {'conv2d': 1} and _counts(cases['default dil64']) == {'conv2d': 4}


def test_routes_match_fixture(routes):
    cases, _ = routes
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert sorted(gold['cases']) == sorted(cases)
    for key, log in cases.items():
        want = [gold['records'][i] for i in gold['cases'][key]]
        assert log == want, '{}: first difference at launch {}'.format(
            key, next((i for i, (a, b) in enumerate(zip(log, want)) if a != b), min(len(log), len(want))))


def test_route_names_the_launch(routes):
    """`_Conv.route` (no tensors, no launch) names the launcher each layer of the default head went to."""
    import sc2bench_amd
    hip = sc2bench_amd.hip
    cases, nets = routes
    seen = set()
    for rec in cases['default head']:
        f = rec.split(' ')
        if f[0] in ('pair', 'avgpool', 'fc'):
            continue
        x_shape = tuple(int(v) for v in f[2].split('x'))
        if f[0] == 'conv2d':
            name, epilogue, has_ep_x = 'tile', int(f[8][3:]), f[9] == 'epx1'
        else:
            name, has_ep_x = f[0], f[6] == 'res1'
            epilogue = hip.EPI_BIAS_ADD_RELU if has_ep_x else hip.EPI_BIAS_RELU if f[5] == 'relu1' else hip.EPI_BIAS
        assert nets.rec.convs[f[1]].route(x_shape, epilogue, has_ep_x, False) == name, rec
        seen.add(name)
    assert seen == {'w8', 'win1', 'stream', 'win3', 'tile'}


def test_one_device_copy_per_layout(routes):
    """After a forward of the default-policy head no layer holds two tensors of equal contents (the pair launch's W1 is the layer's
    own fragment layout, the eight-wave kernel's stream is the window-plane 1x1 kernel's)."""
    _, nets = routes
    n = 0
    for blk in nets.head.blocks:
        for c in blk:
            if c is None:
                continue
            assert set(c._packed) <= {'tile', 'frag', 'win'}
            held = [t for t in list(vars(c).values()) + list(c._packed.values()) if isinstance(t, torch.Tensor)]
            n += len(held)
            for i, a in enumerate(held):
                for b in held[i + 1:]:
                    assert a is not b and not (a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)), c.tag
    assert n > 4 * 52


if __name__ == '__main__':
    assert sys.argv[1:] == ['--write']
    sys.path.insert(0, ROOT)
    import sc2bench_amd
    mp = pytest.MonkeyPatch()
    try:
        got, _ = record_cases(sc2bench_amd.hip, mp)
    finally:
        mp.undo()
    with open(GOLDEN, 'w') as f:
        json.dump(_encode(got), f, separators=(',', ':'))
        f.write('\n')
    print('{}: {} cases, {} bytes'.format(GOLDEN, len(got), os.path.getsize(GOLDEN)))
