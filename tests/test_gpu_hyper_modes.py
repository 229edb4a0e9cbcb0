"""-m gpu: the f32-grade codec modes of the hyperprior bottlenecks (`set_encoder_precision('f32' | 'bf16x3' | 'bf16x6')` on
SHPBasedResNetBottleneck / MSHPBasedResNetBottleneck) against the CPU oracle, whose f32 chain is what the reference computes.

Models: the mshp224 model of benchlib.workloads.build_workload and an SHP twin shaped the same way (the one-headed h_s tail scaled
by abs() * 5 as a whole); the oracle is built from their state dicts.  Inputs: the first 16 images of synthetic_batch(seed 0).

Stage-wise (g_a on x, h_a on the oracle's y, h_s on the oracle's z_hat), per mode: with e_R the restatement's own error of the
stage against the oracle over max|ref| (tests/ref_split_hyper.py, computed here on the CPU) and
    delta = max(4e-6, 3 e_R) * max|ref|
(4e-6: the project's GDN_TOL; the factor 3 for the device summing the same exact products in another order than the restatement),
(a) |device - oracle| <= delta everywhere, (b) z symbols, indexes and y symbols EQUAL the oracle's on every element whose oracle
value lies farther than delta from a rounding tie / a scale-table boundary, and the share of elements (b) leaves out is at most
1e-3 (symbols) / 2e-3 (indexes): a larger e_R fails the cap instead of widening the excuse.

End to end, per mode: for every image whose three integer tensors equal the oracle's, both strings of encode() equal the oracle's
byte for byte; the number of such images is at least half the restatement's own (which must be >= 4 of 16 for 'f32' / 'bf16x6').
Each test prints its figures."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_split_hyper as rh  # noqa: E402

NAMES = ('MSHPBasedResNetBottleneck', 'SHPBasedResNetBottleneck')
PRECISE = {'f32': 'f64', 'bf16x3': 2, 'bf16x6': 3}      # codec mode -> the restatement's arithmetic
N_IMAGES = 16
FLOOR = 4e-6
CAP_SYMBOLS, CAP_INDEXES = 1e-3, 2e-3
_WORLDS = {}


class World(object):
    """One class's device bottleneck, its oracle, the inputs and the oracle's chain; restatements and device runs cached per mode."""

    def __init__(self, S, R, dev, name):
        from benchlib.model import synthetic_batch
        from benchlib.workloads import build_workload
        if name.startswith('MSHP'):
            model = build_workload('mshp224', dev, N_IMAGES)[0]
            self.bl = model.bottleneck_layer
        else:
            torch.manual_seed(0)
            self.bl = rh.shape_like_bench(S.get_layer(name)).eval().to(dev)
            self.bl.update()
        assert type(self.bl).__name__ == name and self.bl.encoder_precision == 'bf16'
        self.ref = getattr(R, name)()
        sd = {k: v.detach().cpu().clone() for k, v in self.bl.state_dict().items()}
        own = self.ref.state_dict()
        self.ref.load_state_dict({k: v for k, v in sd.items() if k in own and own[k].shape == v.shape}, strict=False)
        for k, v in self.ref.named_parameters():
            assert torch.equal(v.detach(), sd[k]), k
        self.ref.eval()
        self.ref.update()
        assert torch.equal(self.bl.entropy_bottleneck._quantized_cdf.cpu(), self.ref.entropy_bottleneck._quantized_cdf)
        assert torch.equal(self.bl.gaussian_conditional._quantized_cdf.cpu(), self.ref.gaussian_conditional._quantized_cdf)
        self.dev = dev
        self.x = synthetic_batch(N_IMAGES, torch.device('cpu'), seed=0)
        self.xd = self.x.to(dev)
        self.oracle = rh.stages(self.ref, self.x, 'f32')
        self._rest, self._front, self._enc = {}, {}, {}

    def restatement(self, mode):
        """-> (stage-wise dict: each stage on the oracle's input, end-to-end dict) in the arithmetic of `mode`."""
        if mode not in self._rest:
            stage_wise = rh.stages(self.ref, self.x, PRECISE[mode], inputs=self.oracle)
            self._rest[mode] = (stage_wise, rh.stages(self.ref, self.x, PRECISE[mode], y=stage_wise['y']))
        return self._rest[mode]

    def front(self, mode):
        """The device's (z symbols, indexes, y symbols) of the 16 images in `mode`, as CPU int32 tensors shaped like the oracle's."""
        if mode not in self._front:
            self.bl.set_encoder_precision(mode)
            try:
                with torch.no_grad():
                    (y_sym, idx, z_sym), _ = self.bl.stage_front(self.xd)
            finally:
                self.bl.set_encoder_precision('bf16')
            o = self.oracle
            self._front[mode] = (z_sym.cpu().view(o['z_sym'].shape), idx.cpu().view(o['idx'].shape), y_sym.cpu().view(o['y_sym'].shape))
        return self._front[mode]

    def oracle_ints(self):
        return self.oracle['z_sym'], self.oracle['idx'], self.oracle['y_sym']


@pytest.fixture(scope='module', params=NAMES)
def world(request, S, R, dev):
    name = request.param
    if name not in _WORLDS:
        _WORLDS[name] = World(S, R, dev, name)
    w = _WORLDS[name]
    yield w
    w.bl.set_encoder_precision('bf16')


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def _tie_distance(t):
    """distance of every element of t from the nearest rounding tie (k + 0.5)"""
    return ((t - torch.floor(t)) - 0.5).abs()


@pytest.mark.parametrize('mode', list(PRECISE))
def test_stage_wise(S, world, mode):
    w, o, dev = world, world.oracle, world.dev
    bl, ref = w.bl, w.ref
    eb, gc = bl.entropy_bottleneck, bl.gaussian_conditional
    mshp = rh.is_mean_scale(ref)
    rs = w.restatement(mode)[0]
    bl.set_encoder_precision(mode)
    with torch.no_grad():
        y_d = bl.analysis(w.xd)
        z_d = bl.hyper_analysis(o['y'].to(dev))
        p_d = bl.hyper_synthesis(bl._z_hat_nhwc(o['z_hat'].to(dev)))
        sc_d, _ = bl._params(p_d)
        z_sym = eb.symbols_device(z_d).cpu().view(o['z_sym'].shape)
        idx = gc.build_indexes(sc_d).cpu()
        mu_d = None if o['means'] is None else o['means'].to(dev)
        y_sym = gc.symbols_indexes_device(y_d, sc_d, mu_d)[0].cpu().view(o['y_sym'].shape)
    bl.set_encoder_precision('bf16')
    tag = '{} {}'.format(type(bl).__name__[:4], mode)
    delta = {}
    for stage, got, want, rest in (('g_a', y_d, o['y'], rs['y']), ('h_a', z_d, o['z'], rs['z']), ('h_s', p_d, o['params'], rs['params'])):
        e_r, e_d = _rel(rest, want), _rel(got.cpu(), want)
        scale = want.abs().max().item()
        delta[stage] = max(FLOOR, 3 * e_r) * scale
        print('{} {}: restatement error {:.2e}, device error {:.2e} of max|ref| {:.3g} (delta {:.2e} of it)'.format(
            tag, stage, e_r, e_d, scale, delta[stage] / scale))
        assert e_d * scale <= delta[stage], '(a) {} {}: device error {} > delta {}'.format(tag, stage, e_d, delta[stage] / scale)
    # (b): the integers, away from the ties / boundaries of the ORACLE's values
    med = ref._get_means(o['z'])
    safe_z = _tie_distance(o['z'] - med) > delta['h_a']
    safe_y = _tie_distance(o['y'] - (o['means'] if mshp else 0.0)) > delta['g_a']
    near = torch.zeros_like(o['scales'], dtype=torch.bool)
    for t in ref.gaussian_conditional.scale_table[:-1]:
        near |= (o['scales'] - t).abs() <= delta['h_s']
    safe_i = ~near
    for what, got, want, safe, cap in (('z symbols', z_sym, o['z_sym'], safe_z, CAP_SYMBOLS), ('indexes', idx, o['idx'], safe_i, CAP_INDEXES),
                                      ('y symbols', y_sym, o['y_sym'], safe_y, CAP_SYMBOLS)):
        left_out = 1.0 - safe.float().mean().item()
        differ = (got != want)
        print('{} {}: {} of {} differ ({:.2e}); left out as near a tie / boundary {:.2e} (cap {:.0e})'.format(
            tag, what, int(differ.sum()), differ.numel(), differ.float().mean().item(), left_out, cap))
        assert left_out <= cap, '{} {}: {} of the elements lie within delta of a tie (cap {})'.format(tag, what, left_out, cap)
        assert not bool((differ & safe).any()), '(b) {} {}: {} elements differ away from every tie'.format(tag, what, int((differ & safe).sum()))


def _device_encode(w, mode):
    if mode not in w._enc:
        w.bl.set_encoder_precision(mode)
        try:
            with torch.no_grad():
                w._enc[mode] = w.bl.encode(w.xd)
        finally:
            w.bl.set_encoder_precision('bf16')
    return w._enc[mode]


@pytest.mark.parametrize('mode', list(PRECISE))
def test_end_to_end_bytes(S, world, mode):
    w, ref = world, world.ref
    want = w.oracle_ints()
    same = rh.identical_images(w.front(mode), want)
    rest = w.restatement(mode)[1]
    same_rest = rh.identical_images((rest['z_sym'], rest['idx'], rest['y_sym']), want)
    n, n_rest = sum(same), sum(same_rest)
    print('{} {}: {} of {} images with all three integer tensors equal to the oracle\'s (restatement: {})'.format(
        type(w.bl).__name__[:4], mode, n, N_IMAGES, n_rest))
    # the bytes of those images ARE the oracle's
    enc = _device_encode(w, mode)
    if 'enc' not in w.__dict__:
        with torch.no_grad():
            w.enc = ref.encode(w.x)
    assert tuple(enc['shape']) == tuple(w.enc['shape'])
    ids = [i for i in range(N_IMAGES) if same[i]]
    for i in ids:
        assert enc['strings'][0][i] == w.enc['strings'][0][i], 'image {}: y string differs from the oracle\'s'.format(i)
        assert enc['strings'][1][i] == w.enc['strings'][1][i], 'image {}: z string differs from the oracle\'s'.format(i)
    if ids:     # ... and carry the oracle's latent: its decoder on the device's bytes = its synthesis of its own dequantised latent
        with torch.no_grad():
            dec = ref.decode([[enc['strings'][0][i] for i in ids], [enc['strings'][1][i] for i in ids]], enc['shape'])
            o = w.oracle
            y_hat = ref.gaussian_conditional.quantize(o['y'][ids], 'dequantize', None if o['means'] is None else o['means'][ids])
            assert torch.equal(dec, ref.g_s(y_hat))
    if mode in ('f32', 'bf16x6'):
        assert n_rest >= 4, 'inconclusive: the restatement itself codes only {} of {} images to the oracle\'s integers'.format(n_rest, N_IMAGES)
        assert n >= n_rest // 2
    else:
        assert n >= n_rest // 2 and (n > 0 or n_rest <= 1)


def test_mismatch_rates_are_ordered(S, world):
    """y symbols against the oracle's: rate('bf16x6') <= rate('bf16x3') < rate('bf16') / 100 (as the FP bottleneck's test)."""
    want = world.oracle['y_sym']
    rate = {}
    for mode in ('bf16', 'f32', 'bf16x3', 'bf16x6'):
        got = world.front(mode)
        rate[mode] = (got[2] != want).float().mean().item()
        print('{} {}: mismatch rates z symbols {:.2e}, indexes {:.2e}, y symbols {:.2e}; identical images {}'.format(
            type(world.bl).__name__[:4], mode, (got[0] != world.oracle['z_sym']).float().mean().item(),
            (got[1] != world.oracle['idx']).float().mean().item(), rate[mode], sum(rh.identical_images(got, world.oracle_ints()))))
    assert rate['bf16x6'] <= rate['bf16x3'] < rate['bf16'] / 100


@pytest.mark.parametrize('mode', list(PRECISE))
def test_self_consistency(S, world, mode):
    w, bl, hip = world, world.bl, S.hip
    gc = bl.gaussian_conditional
    x = w.xd[:3]
    with torch.no_grad():
        bf16_before = bl.encode(x)['strings']
        bl.set_encoder_precision(mode)
        (y_sym, idx, z_sym), meta = bl.stage_front(x)
        enc = bl.encode(x)
        out = bl.decode(**enc)
        # decode = synthesis of the dequantised latent (the means from this mode's h_s on the dequantised z)
        (h, wd), z_shape = meta
        params = bl.hyper_synthesis(bl._z_hat_from_symbols(z_sym, z_shape))
        sc, mu = bl._params(params)
        C = y_sym.shape[1] // (h * wd)
        y_hat = hip.gc_dequantize(y_sym.view(3, C, h, wd), None if mu is None else mu.float(), want_f32=False, want_nhwc=True)[1]
        assert torch.equal(out, bl.synthesis_nhwc(y_hat))
        assert torch.equal(bl(x), out)                                  # forward() in updated-eval mode
        # the staged form: the same integers, coder status 0, the same latent and byte counts
        assert torch.equal(gc.build_indexes(sc).view(3, -1), idx)
        y_hat2, nbytes, status = bl.stage_coder((y_sym, idx, z_sym), meta)
        assert int(status.abs().max()) == 0
        assert torch.equal(y_hat2, y_hat)
        assert nbytes.cpu().tolist() == [len(a) + len(b) for a, b in zip(*enc['strings'])]
        assert torch.equal(bl.synthesis_nhwc(bl.stage_decode(y_hat2, meta)), out)
        # batch sizes 1 and 3 agree
        for i in range(3):
            (ys1, id1, zs1), _ = bl.stage_front(x[i:i + 1])
            assert torch.equal(ys1[0], y_sym[i]) and torch.equal(id1[0], idx[i]) and torch.equal(zs1[0], z_sym[i])
            e1 = bl.encode(x[i:i + 1])
            assert e1['strings'][0][0] == enc['strings'][0][i] and e1['strings'][1][0] == enc['strings'][1][i]
            assert torch.equal(bl.decode(**e1), out[i:i + 1])
        # a forced slicing of the batch in g_a (the 2 GB rule) changes nothing
        y_all = bl.analysis(x)
        y_sliced = bl._analysis_f32(x.float(), ns=bl._precise_ns(), slice_bytes=4 * 96 * 112 * 112)
        assert torch.equal(y_all, y_sliced)
        if rh.is_mean_scale(bl):
            bl.train()
            assert torch.equal(bl(x), out)                              # the updated-train path dequantises the same way
            bl.eval()
        # the not-updated likelihood path without grad runs in the mode too
        bl.updated = False
        o2 = bl(x)
        bl.updated = True
        assert o2.shape == out.shape and bl.last_likelihoods[0].shape == (3, C, h, wd)
        bl.set_encoder_precision('bf16')
        assert bl.encode(x)['strings'] == bf16_before                   # after the tour: 'bf16' as it was
