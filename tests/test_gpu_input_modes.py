"""-m gpu: the f32-grade codec modes of the neural input compression models (`set_encoder_precision('f32' | 'bf16x3' | 'bf16x6')` on
FactorizedPrior, ScaleHyperprior and MeanScaleHyperprior of compression.py) against the CPU oracle (oracle.cpu_ref_input /
tests/ref_input_hyperprior.py), whose f32 chain is what the reference computes.  Conventions of tests/test_gpu_hyper_modes.py.

Models and inputs: tests/ref_split_input.py (N = 128, M = 192, 4 images of 128 x 192; y is 8 x 12, z is 2 x 3).

Stage-wise (g_a on x, h_a on the oracle's y, h_s on the oracle's z_hat, g_s on the oracle's y_hat), per mode: with e_R the
restatement's own error of the stage against the oracle over max|ref| (computed here on the CPU) and
    delta = max(4e-6, 3 e_R) * max|ref|
(a) |device - oracle| <= delta everywhere, (b) z symbols, indexes and y symbols EQUAL the oracle's on every element whose oracle
value lies farther than delta from a rounding tie / a scale-table boundary, and the share of elements (b) leaves out is at most
1e-3 (symbols) / 2e-3 (indexes) for 'f32' / 'bf16x6' and 2e-3 / 4e-3 for 'bf16x3': a larger e_R fails the cap instead of widening
the excuse (tests/test_input_modes_cpu.py computes the restatement's own shares).

End to end, every stage fed its own values, per mode: for every image whose integer tensors equal the oracle's, every string of
compress() equals the oracle's byte for byte and decompress() of those strings gives the oracle's x_hat within delta before the
clamp (delta from the END-TO-END restatement's x_hat of those images, the same rule); the number of such images is at least half
the restatement's own, which must be >= 2 of 4 for 'f32' / 'bf16x6'.  Each test prints its figures."""
import os
import sys

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_split_input as ri  # noqa: E402

PRECISE = {'f32': 'f64', 'bf16x3': 2, 'bf16x6': 3}      # codec mode -> the restatement's arithmetic
FLOOR = 4e-6
CAP_SYMBOLS = {'f32': 1e-3, 'bf16x6': 1e-3, 'bf16x3': 2e-3}
CAP_INDEXES = {'f32': 2e-3, 'bf16x6': 2e-3, 'bf16x3': 4e-3}
_WORLDS = {}


class World(object):
    """One class's device model, its oracle, the inputs and the oracle's chain; restatements and device runs cached per mode."""

    def __init__(self, S, dev, name):
        self.ref = ri.build(name)
        self.m = S.COMPRESSION_MODEL_CLASS_DICT[name](ri.N_CH, ri.M_CH)
        self.m.load_state_dict({k: v.clone() for k, v in self.ref.state_dict().items()})
        self.m.eval().to(dev)
        assert type(self.m).__name__ == name and self.m.encoder_precision == 'bf16'
        assert torch.equal(self.m.entropy_bottleneck._quantized_cdf.cpu(), self.ref.entropy_bottleneck._quantized_cdf)
        self.hyper = ri.has_hyper(self.ref)
        if self.hyper:
            assert torch.equal(self.m.gaussian_conditional._quantized_cdf.cpu(), self.ref.gaussian_conditional._quantized_cdf)
        self.dev = dev
        self.x = ri.images()
        self.xd = self.x.to(dev)
        self.oracle = ri.stages(self.ref, self.x, 'f32')     # (each stage on its own values: the oracle's chain)
        with torch.no_grad():
            self.enc = self.ref.compress(self.x)
        self._rest, self._run = {}, {}

    def restatement(self, mode):
        """-> (stage-wise dict: each stage on the oracle's input, end-to-end dict) in the arithmetic of `mode`."""
        if mode not in self._rest:
            stage_wise = ri.stages(self.ref, self.x, PRECISE[mode], inputs=self.oracle)
            self._rest[mode] = (stage_wise, ri.stages(self.ref, self.x, PRECISE[mode], y=stage_wise['y']))
        return self._rest[mode]

    def run(self, mode):
        """compress() of the 4 images in `mode` and the integer tensors behind its strings (CPU int32, shaped like the oracle's)."""
        if mode not in self._run:
            m, o = self.m, self.oracle
            m.set_encoder_precision(mode)
            try:
                with torch.no_grad():
                    enc = m.compress(self.xd)
                    y = m.analysis(self.xd)
                    if self.hyper:
                        gc = m.gaussian_conditional
                        z_sym = m.entropy_bottleneck.symbols_device(m.hyper_analysis(y)).cpu().view(o['z_sym'].shape)
                        scales, means = m._gaussian(m.hyper_synthesis(m._z_hat_nhwc(enc['strings'][1], enc['shape'])))
                        ints = (z_sym, gc.build_indexes(scales).cpu().int(), gc.quantize(y, 'symbols', means).cpu().int())
                    else:
                        ints = (m.entropy_bottleneck.symbols_device(y).cpu().view(o['y_sym'].shape),)
            finally:
                m.set_encoder_precision('bf16')
            self._run[mode] = (enc, ints)
        return self._run[mode]


@pytest.fixture(scope='module', params=ri.NAMES)
def world(request, S, dev):
    name = request.param
    if name not in _WORLDS:
        _WORLDS[name] = World(S, dev, name)
    w = _WORLDS[name]
    yield w
    w.m.set_encoder_precision('bf16')


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def _tie_distance(t):
    """distance of every element of t from the nearest rounding tie (k + 0.5)"""
    return ((t - torch.floor(t)) - 0.5).abs()


@pytest.mark.parametrize('mode', list(PRECISE))
def test_stage_wise(S, world, mode):
    w, o, dev = world, world.oracle, world.dev
    m, ref = w.m, w.ref
    eb = m.entropy_bottleneck
    rs = w.restatement(mode)[0]
    m.set_encoder_precision(mode)
    with torch.no_grad():
        got = {'g_a': m.analysis(w.xd), 'g_s': m.synthesis(o['y_hat'].to(dev))}
        if w.hyper:
            gc = m.gaussian_conditional
            got['h_a'] = m.hyper_analysis(o['y'].to(dev))
            got['h_s'] = m.hyper_synthesis(m._nhwc(o['z_hat'].to(dev)))
            sc_d, _ = m._gaussian(got['h_s'])
            z_sym = eb.symbols_device(got['h_a']).cpu().view(o['z_sym'].shape)
            idx = gc.build_indexes(sc_d).cpu().int()
            mu_d = None if o['means'] is None else o['means'].to(dev)
            y_sym = gc.quantize(got['g_a'], 'symbols', mu_d).cpu().int()
        else:
            y_sym = eb.symbols_device(got['g_a']).cpu().view(o['y_sym'].shape)
    m.set_encoder_precision('bf16')
    tag = '{} {}'.format(type(m).__name__, mode)
    keys = {'g_a': 'y', 'h_a': 'z', 'h_s': 'params', 'g_s': 'x_hat'}
    delta = {}
    for stage in ('g_a', 'h_a', 'h_s', 'g_s'):
        if stage not in got:
            continue
        want, rest = o[keys[stage]], rs[keys[stage]]
        assert got[stage].dtype == torch.float32 and tuple(got[stage].shape) == tuple(want.shape)
        e_r, e_d = _rel(rest, want), _rel(got[stage].cpu(), want)
        scale = want.abs().max().item()
        delta[stage] = max(FLOOR, 3 * e_r) * scale
        print('{} {}: restatement error {:.2e}, device error {:.2e} of max|ref| {:.3g} (delta {:.2e} of it)'.format(
            tag, stage, e_r, e_d, scale, delta[stage] / scale))
        assert e_d * scale <= delta[stage], '(a) {} {}: device error {} > delta {}'.format(tag, stage, e_d, delta[stage] / scale)
    # (b): the integers, away from the ties / boundaries of the ORACLE's values
    checks = []
    if w.hyper:
        safe_z = _tie_distance(o['z'] - ri.medians(ref.entropy_bottleneck, o['z'])) > delta['h_a']
        safe_y = _tie_distance(o['y'] - (o['means'] if o['means'] is not None else 0.0)) > delta['g_a']
        near = torch.zeros_like(o['scales'], dtype=torch.bool)
        for t in ref.gaussian_conditional.scale_table[:-1]:
            near |= (o['scales'] - t).abs() <= delta['h_s']
        checks = [('z symbols', z_sym, o['z_sym'], safe_z, CAP_SYMBOLS[mode]), ('indexes', idx, o['idx'], ~near, CAP_INDEXES[mode])]
    else:
        safe_y = _tie_distance(o['y'] - ri.medians(ref.entropy_bottleneck, o['y'])) > delta['g_a']
    checks.append(('y symbols', y_sym, o['y_sym'], safe_y, CAP_SYMBOLS[mode]))
    for what, have, want, safe, cap in checks:
        left_out = 1.0 - safe.float().mean().item()
        differ = (have != want)
        print('{} {}: {} of {} differ ({:.2e}); left out as near a tie / boundary {:.2e} (cap {:.0e})'.format(
            tag, what, int(differ.sum()), differ.numel(), differ.float().mean().item(), left_out, cap))
        assert left_out <= cap, '{} {}: {} of the elements lie within delta of a tie (cap {})'.format(tag, what, left_out, cap)
        assert not bool((differ & safe).any()), '(b) {} {}: {} elements differ away from every tie'.format(tag, what, int((differ & safe).sum()))


def _device_y_hat(w, strings, shape):
    """y_hat f32 NCHW as decompress() rebuilds it from `strings` (the model is in the mode under test)."""
    m = w.m
    if not w.hyper:
        return m.entropy_bottleneck.decompress(strings[0], tuple(shape))
    gc = m.gaussian_conditional
    scales, means = m._gaussian(m.hyper_synthesis(m._z_hat_nhwc(strings[1], shape)))
    return gc.decompress(strings[0], gc.build_indexes(scales), means=means)


@pytest.mark.parametrize('mode', list(PRECISE))
def test_end_to_end_bytes(S, world, mode):
    w, ref, m = world, world.ref, world.m
    o = w.oracle
    want = ri.int_tensors(o)
    enc, ints = w.run(mode)
    same = ri.identical_images(ints, want)
    rest = w.restatement(mode)[1]
    same_rest = ri.identical_images(ri.int_tensors(rest), want)
    n, n_rest = sum(same), sum(same_rest)
    print('{} {}: {} of {} images with all integer tensors equal to the oracle\'s (restatement: {})'.format(
        type(m).__name__, mode, n, ri.N_IMAGES, n_rest))
    assert tuple(enc['shape']) == tuple(w.enc['shape']) and len(enc['strings']) == len(w.enc['strings'])
    ids = [i for i in range(ri.N_IMAGES) if same[i]]
    for i in ids:       # the bytes of those images ARE the oracle's
        for k, (have, theirs) in enumerate(zip(enc['strings'], w.enc['strings'])):
            assert have[i] == theirs[i], 'image {}: string {} differs from the oracle\'s'.format(i, k)
    if ids:             # ... and decode to the oracle's reconstruction
        sub = [[s[i] for i in ids] for s in enc['strings']]
        m.set_encoder_precision(mode)
        try:
            with torch.no_grad():
                out = m.decompress(sub, enc['shape'])['x_hat']
                pre = m.synthesis(_device_y_hat(w, sub, enc['shape']))
        finally:
            m.set_encoder_precision('bf16')
        assert torch.equal(out, pre.clamp(0, 1))                     # decompress = the clamp of this reconstruction
        x_hat = o['x_hat'][ids]
        scale = x_hat.abs().max().item()
        e_r, e_d = _rel(rest['x_hat'][ids], x_hat), _rel(pre.cpu(), x_hat)
        delta = max(FLOOR, 3 * e_r)
        print('{} {}: x_hat of {} images before the clamp: restatement error {:.2e}, device error {:.2e} of max|ref| {:.3g} '
              '(delta {:.2e})'.format(type(m).__name__, mode, len(ids), e_r, e_d, scale, delta))
        assert e_d <= delta
    if mode in ('f32', 'bf16x6'):
        assert n_rest >= 2, 'inconclusive: the restatement itself codes only {} of {} images to the oracle\'s integers'.format(n_rest, ri.N_IMAGES)
    assert n >= n_rest // 2


@pytest.mark.parametrize('mode', list(PRECISE))
def test_staged_equals_round_trip(S, dev, mode):
    """FactorizedPrior: stage_front -> stage_coder(dequantized=True) -> stage_back in a precise mode = decompress(compress(x)) of
    that mode, bit for bit; the coder hands on symbols, never a bf16 latent."""
    if 'FactorizedPrior' not in _WORLDS:
        _WORLDS['FactorizedPrior'] = World(S, dev, 'FactorizedPrior')
    w = _WORLDS['FactorizedPrior']
    m = w.m
    m.set_encoder_precision(mode)
    try:
        with torch.no_grad():
            want = m.decompress(**m.compress(w.xd))['x_hat']
            sym, hw = m.stage_front(w.xd)
            decoded, nbytes, status = m.stage_coder(sym, hw, dequantized=True)
            assert decoded.dtype == torch.int32 and int(status.abs().max()) == 0
            got = m.stage_back(decoded, hw)
            assert torch.equal(got, want)
            assert torch.equal(m(w.xd)['x_hat'].clamp(0, 1), want)          # forward() in eval: the same reconstruction before the clamp
            with pytest.raises(S.hip.Sc2Error):
                m.stage_back(torch.zeros(1, 8, 12, ri.M_CH, dtype=torch.bfloat16, device=dev), hw)
    finally:
        m.set_encoder_precision('bf16')


@pytest.mark.parametrize('mode', list(PRECISE))
def test_forced_slices_are_bit_identical(S, world, mode):
    """slice_bytes forced down to one image's widest map: the 4 images run as 4 slices and give the unsliced tensors."""
    from sc2bench_amd.entropy import _precise_geometry, run_hip_transform_precise
    w, m, o = world, world.m, world.oracle
    m.set_encoder_precision(mode)
    ns = m._precise_ns()
    one = 4 * ri.N_CH * 64 * 96            # g_a's first map / g_s's last 128-channel map of ONE image, in bytes
    try:
        with torch.no_grad():
            y = m.analysis(w.xd)
            assert torch.equal(m.analysis(w.xd, slice_bytes=one), y)
            assert torch.equal(m.analysis(w.xd, slice_bytes=2 * one + 5), y)       # slices of 2
            y_hat = o['y_hat'].to(w.dev)
            assert torch.equal(m.synthesis(y_hat, slice_bytes=one), m.synthesis(y_hat))
            if w.hyper:
                z_hat = m._nhwc(o['z_hat'].to(w.dev))
                widest = 4 * max(h * wd * c for _, h, wd, c in _precise_geometry(list(m.h_s), (1,) + tuple(z_hat.shape[1:])))
                assert torch.equal(run_hip_transform_precise(m.h_s, z_hat, ns, slice_bytes=widest), m.hyper_synthesis(z_hat))
    finally:
        m.set_encoder_precision('bf16')


def test_bf16_is_untouched_by_a_round_trip_through_the_modes(S, world):
    w, m = world, world.m
    x = w.xd[:2]
    with torch.no_grad():
        before = m.compress(x)
        x_hat = m.decompress(**before)['x_hat']
        fwd = m(x)['x_hat']
        assert x_hat.dtype == torch.float32
        for mode in PRECISE:
            m.set_encoder_precision(mode)
            out = m.decompress(**m.compress(x))['x_hat']
            assert out.shape == x_hat.shape
        m.set_encoder_precision('bf16')
        after = m.compress(x)
        assert after['strings'] == before['strings'] and tuple(after['shape']) == tuple(before['shape'])
        assert torch.equal(m.decompress(**after)['x_hat'], x_hat)
        assert torch.equal(m(x)['x_hat'], fwd)


def test_walker_raises_instead_of_falling_back(S, dev):
    from sc2bench_amd.entropy import run_hip_transform_precise
    hip = S.hip
    x = torch.zeros(1, 4, 4, 8, device=dev)
    conv = S.HipConv2d(8, 8, 3, padding=1).to(dev)
    for seq in (nn.Sequential(conv, nn.Sigmoid()), nn.Sequential(conv, nn.LeakyReLU(0.2)), nn.Sequential(nn.Conv2d(8, 8, 1).to(dev)),
                nn.Sequential(S.HipConv2d(8, 8, 3, padding=1, groups=2).to(dev))):
        with pytest.raises(hip.Sc2Error):
            run_hip_transform_precise(seq, x, 0)
    with pytest.raises(hip.Sc2Error):
        run_hip_transform_precise(nn.Sequential(conv), x, 0, out_format=hip.OUT_BF16_NHWC)
    with pytest.raises(hip.Sc2Error):
        run_hip_transform_precise(nn.Sequential(conv), x.to(torch.bfloat16), 0)
    with pytest.raises(hip.Sc2Error):
        run_hip_transform_precise(nn.Sequential(conv), x, 5)
    # run_hip_sequence_precise keeps refusing a GDN
    from sc2bench_amd.entropy import run_hip_sequence_precise
    with pytest.raises(hip.Sc2Error):
        run_hip_sequence_precise(nn.Sequential(S.GDN(8).to(dev)), x, 0)
