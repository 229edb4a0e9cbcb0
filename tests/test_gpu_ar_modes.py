"""-m gpu: the codec modes of mbt2018 (JointAutoregressiveHierarchicalPriors.set_scan_precision / set_encoder_precision) on the
device against the oracle (tests/ref_input_hyperprior.py) at the operating point of tests/ref_ar_modes.py, whose reference-alone
conditions are checked in tests/test_ar_modes_cpu.py.

For the scan 'f32' with the encoder 'bf16', and for each precise encoder mode: the round trip is bit exact, the strings are the
oracle coder's on the device's integers, the scan lies within the derived f32 bound of the float64 step on the model's own f32
pack (tests/ref_ar_scan.py).  Precise modes: every stage within delta = max(4e-6, 3 e_R) max|ref| of the oracle's f32 chain, e_R
from the CPU restatement of the stage in the mode's arithmetic (ref_split_input.run_seq), the rule of tests/test_gpu_input_modes.py;
and every image the device codes to the oracle's integers has the oracle's bytes and decodes to the oracle's x_hat within delta.

The bf16 cases need the bf16 transforms at N = 32: the squared-form GDN of a narrow layer (tests/test_gpu_narrow_gdn.py).
Measured on an MI355X: 'f32' and 'bf16x6' code 4 of 4 images to the oracle's integers and bytes, 'bf16x3' 3 of 4; the scan's
largest |err| / bound stays below 1e-3."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_ar_modes as RM  # noqa: E402
import ref_ar_scan as RA  # noqa: E402
import ref_split_input as ri  # noqa: E402

FLOOR = 4e-6
CONFIGS = [('f32', 'bf16'), ('f32', 'f32'), ('f32', 'bf16x3'), ('f32', 'bf16x6')]      # (scan, encoder)
MODES = list(RM.PRECISE)


class World(object):
    def __init__(self, S, dev):
        self.ref, self.x, self.o = RM.world()
        ref = self.ref
        self.m = S.COMPRESSION_MODEL_CLASS_DICT['JointAutoregressiveHierarchicalPriors'](RM.N_CH, RM.M_CH)
        self.m.load_state_dict({k: v.clone() for k, v in ref.state_dict().items()})
        self.m.eval().to(dev)
        m = self.m
        assert (m.scan_precision, m.encoder_precision) == ('bf16', 'bf16')
        assert torch.equal(m.gaussian_conditional._quantized_cdf.cpu(), ref.gaussian_conditional._quantized_cdf)
        assert torch.equal(m.entropy_bottleneck._quantized_cdf.cpu(), ref.entropy_bottleneck._quantized_cdf)
        self.dev = dev
        self.xd = self.x.to(dev)
        self._bf16_before = None
        self._o64 = None

    def bf16_before(self):
        """compress() in 'bf16' / 'bf16'; the first call is made before any test of this module sets a mode (the fixture below)."""
        if self._bf16_before is None:
            assert (self.m.scan_precision, self.m.encoder_precision) == ('bf16', 'bf16')
            with torch.no_grad():
                self._bf16_before = self.m.compress(self.xd)
        return self._bf16_before

    def o64(self):
        """The float64 evaluation of the oracle (the CPU test: it reproduces the f32 oracle's integers on every image)."""
        if self._o64 is None:
            self._o64 = RM.chain(copy.deepcopy(self.ref).double(), self.x)
        return self._o64

    def set(self, scan, encoder):
        self.m.set_encoder_precision('bf16').set_scan_precision(scan).set_encoder_precision(encoder)

    def reset(self):
        self.m.set_encoder_precision('bf16').set_scan_precision('bf16')


_WORLD = []


@pytest.fixture(scope='module')
def world(S, dev):
    if not _WORLD:
        _WORLD.append(World(S, dev))
        try:
            _WORLD[0].bf16_before()
        except S.hip.Sc2Error as e:      # the tests that need the bf16 transforms report it themselves
            print('bf16 / bf16 compress at the operating point: {}'.format(e))
    yield _WORLD[0]
    _WORLD[0].reset()


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def _tables(gc):
    return gc._quantized_cdf.cpu().numpy(), gc._cdf_length.cpu().numpy(), gc._offset.cpu().numpy()


# --------------------------------------------------------------------------------------------- #
# round trip and scan, every configuration
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('scan,encoder', CONFIGS, ids=lambda v: v)
def test_round_trip_and_scan(S, world, scan, encoder):
    from oracle import rans as oracle_rans
    w, m, dev = world, world.m, world.dev
    gc = m.gaussian_conditional
    M, B = m.M, w.xd.shape[0]
    w.set(scan, encoder)
    try:
        with torch.no_grad():
            H, W = w.xd.shape[2] // 16, w.xd.shape[3] // 16
            gp = torch.full((B, H * W, 2 * M), float('nan'), dtype=torch.float32, device=dev)
            enc = m.compress_device(w.xd, gaussian_params=gp)
            obj = m.compress(w.xd)
            y_pad, y_hat, sym = m.decompress_device(obj['strings'], obj['shape'])
            assert torch.equal(y_pad, enc['y_hat_pad']) and torch.equal(sym, enc['symbols'])
            y_pad3, y_hat3, sym3 = m.decompress_device(obj['strings'], obj['shape'], chunks=3)
            assert torch.equal(y_pad3, y_pad) and torch.equal(sym3, sym)
            if encoder == 'bf16':
                assert torch.equal(y_hat.float(), y_pad[:, 2:, 2:-2].to(torch.bfloat16).float()) and torch.equal(y_hat3, y_hat)
            else:
                assert y_hat is None and y_hat3 is None          # g_s takes the f32 interior of y_hat_pad
            out = m.decompress(**obj)['x_hat']
            want = y_hat if encoder == 'bf16' else y_pad[:, 2:, 2:-2].contiguous()
            assert torch.equal(out, m.synthesis_nhwc(want).clamp_(0, 1))
            # the strings: the oracle coder on the device's symbols and indexes; z: the oracle's coder on the device's z
            tabs = _tables(gc)
            for i in range(B):
                s, ix = enc['symbols'][i].cpu().numpy(), enc['indexes'][i].cpu().numpy()
                assert obj['strings'][0][i] == oracle_rans.encode_with_indexes(s, ix, *tabs)
                assert np.array_equal(oracle_rans.decode_with_indexes(obj['strings'][0][i], ix, *tabs), s)
            z = m.hyper_analysis(enc['y'])
            assert obj['strings'][1] == w.ref.entropy_bottleneck.compress(z.cpu())
            # batch invariance, as test_mbt2018_batch_invariance
            x = w.xd
            alone = m.compress(x[3:4])
            first = m.compress(torch.cat([x[3:4], x[:3]]))
            for k in (0, 1):
                assert obj['strings'][k][3] == alone['strings'][k][0] == first['strings'][k][0]
            pad_alone = m.decompress_device(alone['strings'], alone['shape'])[0]
            mixed = [[obj['strings'][k][i] for i in (0, 3, 1)] for k in (0, 1)]
            pad_mixed = m.decompress_device(mixed, obj['shape'])[0]
            assert torch.equal(pad_mixed[1], pad_alone[0]) and torch.equal(pad_alone[0], y_pad[3])
            pack = {k: v.cpu().double().numpy() for k, v in m._packed(scan_f32=True)['scan_f32'].items()}
            assert m._scan_weights() is m._packed()['scan_f32']
        # the scan: within the derived f32 bound of the float64 step on the model's own UNROUNDED weights, integers exact given them
        case = {'weights': pack, 'p1': enc['p1'].cpu().double().numpy(), 'y': enc['y'].cpu().numpy(),
                'scale_table': gc.scale_table.cpu().float().numpy(), 'scale_bound': float(gc._scale_bound),
                'shape': (M, pack['w1'].shape[1], pack['w2'].shape[1], H, W, B)}
        assert case['shape'][1:3] == (136, 112) and not pack['w1'][:, 133:].any() and not pack['w3'][106:].any()
        got = {'gaussian_params': gp.cpu().numpy(), 'y_hat_pad': enc['y_hat_pad'].cpu().numpy(),
               'symbols': enc['symbols'].cpu().numpy(), 'indexes': enc['indexes'].cpu().numpy()}
        ratio = RA.assert_random(case, got)
        print('scan {} encoder {}: largest |err| / bound of the scan = {:.4g}; {} distinct indexes'.format(
            scan, encoder, ratio, len(np.unique(got['indexes']))))
        assert ratio < 1
    finally:
        w.reset()


# --------------------------------------------------------------------------------------------- #
# precise modes, stage by stage on the oracle's inputs
# --------------------------------------------------------------------------------------------- #
def _plain_conv(weight, bias, padding=0):
    c = nn.Conv2d(weight.shape[1], weight.shape[0], weight.shape[2], padding=padding)
    with torch.no_grad():
        c.weight.copy_(weight)
        c.bias.copy_(bias)
    return c


def _restated(ref, o, mode):
    """Each stage on the ORACLE's input in the arithmetic of `mode` -> dict stage -> f32 NCHW."""
    arith = RM.PRECISE[mode]
    M = ref.M
    ep, cp = ref.entropy_parameters, ref.context_prediction
    with torch.no_grad():
        p1 = _plain_conv(ep[0].weight[:, :2 * M], ep[0].bias)
        ctx = _plain_conv(cp.weight * cp.mask, cp.bias, padding=2)
        h = torch.cat((o['params'], ri.run_seq([ctx], o['y_hat'], arith)), dim=1)
        return {'g_a': ri.run_seq(ref.g_a, RM.images(), arith), 'h_a': ri.run_seq(ref.h_a, o['y'], arith),
                'h_s': ri.run_seq(ref.h_s, o['z_hat'], arith), 'g_s': ri.run_seq(ref.g_s, o['y_hat'], arith),
                'p1': ri.run_seq([p1], o['params'], arith), 'gp': ri.run_seq(ep, h, arith)}


def _oracle_stages(ref, o):
    M = ref.M
    ep = ref.entropy_parameters
    with torch.no_grad():
        return {'g_a': o['y'], 'h_a': o['z'], 'h_s': o['params'], 'g_s': o['x_hat'],
                'p1': F.conv2d(o['params'], ep[0].weight[:, :2 * M], ep[0].bias), 'gp': ref.gaussian_params(o['params'], o['y_hat'])}


@pytest.mark.parametrize('mode', MODES)
def test_stage_wise(S, world, mode):
    w, m, o, dev = world, world.m, world.o, world.dev
    want, rest = _oracle_stages(w.ref, o), _restated(w.ref, o, mode)
    w.set('f32', mode)
    try:
        with torch.no_grad():
            params_nhwc = m._nhwc(o['params'].to(dev))
            p1 = m.hyper_params_term(params_nhwc)
            got = {'g_a': m.analysis(w.xd), 'h_a': m.hyper_analysis(o['y'].to(dev)),
                   'h_s': m.hyper_synthesis(m._nhwc(o['z_hat'].to(dev))), 'g_s': m.synthesis(o['y_hat'].to(dev)),
                   'p1': p1[..., :133].permute(0, 3, 1, 2),
                   'gp': m.entropy_parameters_nhwc(params_nhwc, m.context_nhwc(o['y_hat'].to(dev)))}
            assert tuple(p1.shape) == (4, 4, 8, 136) and not p1[..., 133:].any()       # the padding columns stay zero
    finally:
        w.reset()
    for stage in ('g_a', 'h_a', 'h_s', 'g_s', 'p1', 'gp'):
        g = got[stage].cpu()
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(want[stage].shape), stage
        e_r, e_d = _rel(rest[stage], want[stage]), _rel(g, want[stage])
        delta = max(FLOOR, 3 * e_r)
        print('mbt2018 {} {}: restatement error {:.2e}, device error {:.2e} of max|ref| {:.3g} (delta {:.2e})'.format(
            mode, stage, e_r, e_d, want[stage].abs().max().item(), delta))
        assert e_d <= delta, '{} {}: device error {} > delta {}'.format(mode, stage, e_d, delta)


# --------------------------------------------------------------------------------------------- #
# precise modes, end to end
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('mode', MODES)
def test_end_to_end_bytes(S, world, mode):
    w, m, o, ref = world, world.m, world.o, world.ref
    B = w.xd.shape[0]
    with torch.no_grad():
        oracle_z = ref.entropy_bottleneck.compress(o['z'])
    w.set('f32', mode)
    try:
        with torch.no_grad():
            enc = m.compress_device(w.xd)
            obj = m.compress(w.xd)
            z_sym = m.entropy_bottleneck.symbols_device(m.hyper_analysis(enc['y'])).cpu().view(o['z_sym'].shape)
            dev_ints = {'z_sym': z_sym, 'idx': enc['indexes'].cpu(), 'y_sym': enc['symbols'].cpu()}
            same = RM.identical_images(dev_ints, o)
            ids = [i for i in range(B) if same[i]]
            print('mbt2018 {}: {} of {} images with z symbols, indexes and y symbols equal to the oracle\'s'.format(mode, len(ids), B))
            for i in ids:                  # their bytes ARE the oracle's
                assert obj['strings'][0][i] == o['strings'][i], 'image {}: the y string differs from the oracle\'s'.format(i)
                assert obj['strings'][1][i] == oracle_z[i], 'image {}: the z string differs from the oracle\'s'.format(i)
            # the round trip holds whatever the count
            y_pad, _, sym = m.decompress_device(obj['strings'], obj['shape'])
            assert torch.equal(y_pad, enc['y_hat_pad']) and torch.equal(sym, enc['symbols'])
            if ids:
                sub = [[s[i] for i in ids] for s in obj['strings']]
                out = m.decompress(sub, obj['shape'])['x_hat']
                pre = m.synthesis_nhwc(m.decompress_device(sub, obj['shape'])[0][:, 2:, 2:-2].contiguous())
                assert torch.equal(out, pre.clamp(0, 1))
    finally:
        w.reset()
    if ids:
        # the end-to-end restatement: g_s in the mode's arithmetic on the y_hat of the float64 oracle (its integers are the
        # oracle's on these images; asserted), against the oracle's f32 x_hat before the clamp
        o64 = w.o64()
        same64 = RM.identical_images(o64, o)
        ids = [i for i in ids if same64[i]]
        assert ids
        x_hat = o['x_hat'][ids]
        rest = ri.run_seq(ref.g_s, o64['y_hat'][ids].float(), RM.PRECISE[mode])
        keep = [k for k, i in enumerate([i for i in range(B) if same[i]]) if same64[i]]
        e_r, e_d = _rel(rest, x_hat), _rel(pre.cpu()[keep], x_hat)
        delta = max(FLOOR, 3 * e_r)
        print('mbt2018 {}: x_hat of {} images before the clamp: restatement error {:.2e}, device error {:.2e} of max|ref| {:.3g} '
              '(delta {:.2e})'.format(mode, len(ids), e_r, e_d, x_hat.abs().max().item(), delta))
        assert e_d <= delta
    if mode in ('f32', 'bf16x6'):
        assert sum(same) >= 3, '{}: only {} of {} images coded to the oracle\'s integers'.format(mode, sum(same), B)


@pytest.mark.parametrize('mode', MODES)
def test_forward_runs_on_the_precise_kernels(S, world, mode):
    """`forward` end to end in a precise mode: the oracle's likelihood bits within 2 % + 16 (the bound of
    test_forward_matches_restatement; y_hat = round(y) may flip at ties), and its Gaussian parameters are the stage-wise ones."""
    w, m, ref = world, world.m, world.ref

    def bits(lik):
        return float((-torch.log2(lik.float().cpu().clamp_min(1e-30))).sum())
    w.set('f32', mode)
    try:
        with torch.no_grad():
            out = m(w.xd)
    finally:
        w.reset()
    with torch.no_grad():
        want = ref(w.x)
    assert out['x_hat'].shape == want['x_hat'].shape and torch.isfinite(out['x_hat']).all()
    for k in ('y', 'z'):
        assert out['likelihoods'][k].shape == want['likelihoods'][k].shape
        b, rb = bits(out['likelihoods'][k]), bits(want['likelihoods'][k])
        print('mbt2018 {} forward: {} bits {:.1f} (oracle {:.1f})'.format(mode, k, b, rb))
        assert abs(b - rb) <= 0.02 * rb + 16, (k, b, rb)


def test_classifier_pass_with_the_precise_codec(S, world):
    from sc2bench_amd import transforms as T
    from sc2bench_amd.resnet import resnet50
    w, m, dev = world, world.m, world.dev
    torch.manual_seed(5)
    clf = resnet50(num_classes=10).eval()
    wrapped = S.NeuralInputCompressionClassifier(
        clf, pre_transform=T.AdaptivePad(fill=0, factor=64), compression_model=m, post_transform=T.Compose([T.CenterCrop([56, 56])]),
        analysis_config={'analyzes_after_compress': True, 'analyzer_configs': [{'key': 'FileSizeAnalyzer', 'kwargs': {'unit': 'KB'}}]})
    wrapped.eval().to(dev)
    wrapped.activate_analysis()
    x = w.xd[:2, :, :56, :56].contiguous()
    w.set('f32', 'f32')
    try:
        with torch.no_grad():
            out = wrapped(x)
            padded = T.AdaptivePad(fill=0, factor=64)(x)
            obj = m.compress(padded)
            x_hat = m.decompress(**obj)['x_hat']
            ref_out = clf(T.CenterCrop([56, 56])(x_hat))
    finally:
        w.reset()
    assert out.shape == (2, 10) and torch.isfinite(out.float()).all()
    # the wrapper ran this very codec: the same x_hat through the classifier's own f32 torch layers, whose library convolutions may sum in
    # another order from call to call (about 50 layers of f32 sums: 1e-4 of the largest logit is far above that and far below a codec change)
    assert (out.float() - ref_out.float()).abs().max().item() <= 1e-4 * ref_out.float().abs().max().item()
    sizes = wrapped.analyzers[0].file_size_list
    assert len(sizes) == 1 and sizes[0] * 1024 >= sum(len(s) for s in obj['strings'][0])


def test_bf16_codec_is_untouched_by_the_modes(S, world):
    """'bf16' / 'bf16' strings before any mode was set (taken when the model was built) and after a run through every mode."""
    w, m = world, world.m
    w.bf16_before()
    with torch.no_grad():
        for scan, encoder in CONFIGS:
            w.set(scan, encoder)
            try:
                other = m.compress(w.xd[:1])
            finally:
                w.reset()
            assert len(other['strings'][0]) == 1
        assert (m.scan_precision, m.encoder_precision) == ('bf16', 'bf16')
        before = w.bf16_before()
        after = m.compress(w.xd)
    assert after['strings'] == before['strings'] and tuple(after['shape']) == tuple(before['shape'])
    assert m._scan_weights() is m._packed()['scan']
