"""The two precision switches of mbt2018 (compression.py: JointAutoregressiveHierarchicalPriors.set_scan_precision /
set_encoder_precision) without a device: every rule of the interface, the f32 scan pack, and the reference-alone condition that
tests/test_gpu_ar_modes.py leans on: at the tests' operating point (tests/ref_ar_modes.py) an f32-grade codec CAN reproduce the
oracle's bytes -- the float64 evaluation of the oracle does, on at least 3 of the 4 images."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_ar_modes as RM  # noqa: E402

PRECISE = ('f32', 'bf16x3', 'bf16x6')


def _model(S, **kw):
    return S.COMPRESSION_MODEL_CLASS_DICT['JointAutoregressiveHierarchicalPriors'](8, 12, **kw)


# ---- the interface ------------------------------------------------------------------------------ #
def test_scan_switch(S):
    m = _model(S)
    assert m.scan_precision == 'bf16' and m.encoder_precision == 'bf16'
    assert m.set_scan_precision('f32') is m and m.scan_precision == 'f32'
    assert m.set_scan_precision('bf16') is m and m.scan_precision == 'bf16'
    for name in ('bf16x3', 'f64', 'fp32', None):
        with pytest.raises(ValueError, match="scan precision must be 'bf16' or 'f32'"):
            m.set_scan_precision(name)
        assert m.scan_precision == 'bf16'


def test_encoder_switch_follows_the_scan_switch(S):
    m = _model(S)
    for mode in PRECISE:                       # scan 'bf16': refused as ever, now naming the way out
        with pytest.raises(S.hip.Sc2Error, match=r"context scan.*set_scan_precision\('f32'\)"):
            m.set_encoder_precision(mode)
        assert m.encoder_precision == 'bf16' and m._precise_ns() is None
    m.set_scan_precision('f32')
    for mode, ns in zip(PRECISE, (0, 2, 3)):
        assert m.set_encoder_precision(mode) is m
        assert m.encoder_precision == mode and m._precise_ns() == ns
        with pytest.raises(S.hip.Sc2Error, match='needs the f32 context scan'):
            m.set_scan_precision('bf16')       # refused while a precise mode is set, and nothing changes
        assert m.scan_precision == 'f32' and m.encoder_precision == mode
        with pytest.raises(ValueError):
            m.set_encoder_precision('f16')
        assert m.encoder_precision == mode
    assert m.set_encoder_precision('bf16') is m and m.set_scan_precision('bf16') is m
    assert (m.scan_precision, m.encoder_precision) == ('bf16', 'bf16')
    # an f32 scan with bf16 transforms is a codec of its own
    assert m.set_scan_precision('f32').encoder_precision == 'bf16'


def test_constructor_and_config_kwargs(S):
    m = _model(S, scan_precision='f32')
    assert (m.scan_precision, m.encoder_precision) == ('f32', 'bf16')
    for mode in PRECISE:
        assert _model(S, scan_precision='f32', encoder_precision=mode).encoder_precision == mode
        assert _model(S, encoder_precision=mode, scan_precision='f32').scan_precision == 'f32'
        with pytest.raises(S.hip.Sc2Error, match='context scan'):
            _model(S, encoder_precision=mode)
        with pytest.raises(S.hip.Sc2Error, match='context scan'):
            _model(S, encoder_precision=mode, scan_precision='bf16')
    with pytest.raises(ValueError):
        _model(S, scan_precision='bf16x3')
    dev = torch.device('cpu')
    for kwargs in ({'quality': 8, 'scan_precision': 'f32', 'encoder_precision': 'f32'},
                   {'encoder_precision': 'f32', 'scan_precision': 'f32', 'quality': 8},
                   {'scan_precision': 'f32', 'quality': 8, 'encoder_precision': 'bf16x6'}):
        m = S.get_compression_model({'key': 'mbt2018', 'kwargs': dict(kwargs), 'update': False}, dev)
        assert type(m).__name__ == 'JointAutoregressiveHierarchicalPriors' and (m.N, m.M) == (192, 320)
        assert (m.scan_precision, m.encoder_precision) == ('f32', kwargs['encoder_precision'])
    plain = S.get_compression_model({'key': 'mbt2018', 'kwargs': {'quality': 1}, 'update': False}, dev)
    assert (plain.scan_precision, plain.encoder_precision) == ('bf16', 'bf16')
    # neither switch is a parameter or a buffer: state dicts are what they were
    both = S.get_compression_model({'key': 'mbt2018', 'kwargs': {'quality': 1, 'scan_precision': 'f32', 'encoder_precision': 'f32'},
                                    'update': False}, dev)
    assert list(both.state_dict()) == list(plain.state_dict())
    assert not any('precision' in k for k in both.state_dict())
    assert not any('precision' in n for n, _ in list(both.named_parameters()) + list(both.named_buffers()))
    plain.load_state_dict(both.state_dict())
    assert (plain.scan_precision, plain.encoder_precision) == ('bf16', 'bf16')
    clone = copy.deepcopy(both)
    assert (clone.scan_precision, clone.encoder_precision) == ('f32', 'f32')


# ---- the f32 scan pack -------------------------------------------------------------------------- #
def _expected_pack(m):
    M = m.M
    ep, cp = m.entropy_parameters, m.context_prediction
    C1, C2 = ep[0].out_channels, ep[2].out_channels
    C1p, C2p = (C1 + 7) // 8 * 8, (C2 + 7) // 8 * 8
    mw = (cp.weight * cp.mask).detach()
    taps = [(ky, kx) for ky in range(2) for kx in range(5)] + [(2, 0), (2, 1)]
    want = {'wc': torch.cat([mw[:, :, ky, kx].t() for ky, kx in taps], 0), 'w1': torch.zeros(2 * M, C1p),
            'w2': torch.zeros(C1p, C2p), 'w3': torch.zeros(C2p, 2 * M)}
    want['w1'][:, :C1] = ep[0].weight.detach()[:, 2 * M:, 0, 0].t()
    want['w2'][:C1, :C2] = ep[2].weight.detach()[:, :, 0, 0].t()
    want['w3'][:C2] = ep[4].weight.detach()[:, :, 0, 0].t()
    return want


def test_f32_scan_pack_is_the_unrounded_masked_weights(S):
    torch.manual_seed(3)
    m = _model(S)                              # M = 12: 10M/3 = 40, 8M/3 = 32 (no padding); and M = 10 below (33 -> 40, 26 -> 32)
    for m in (m, S.COMPRESSION_MODEL_CLASS_DICT['JointAutoregressiveHierarchicalPriors'](8, 10)):
        pk = m._packed()
        assert 'scan_f32' not in pk            # built only when first needed
        assert m._scan_weights() is pk['scan']
        m.set_scan_precision('f32')
        f = m._scan_weights()
        assert f is m._packed()['scan_f32'] and m._packed() is pk and m._scan_weights() is f       # kept with the pack
        want = _expected_pack(m)
        for name in ('wc', 'w1', 'w2', 'w3'):
            assert f[name].dtype == torch.float32 and f[name].is_contiguous()
            assert torch.equal(f[name], want[name]), name                                        # no rounding at all
            assert tuple(f[name].shape) == tuple(pk['scan'][name].shape)
            assert torch.equal(f[name].to(torch.bfloat16), pk['scan'][name])                      # the bf16 pack is its rounding
            assert not torch.equal(f[name], pk['scan'][name].float())
        for name in ('bc', 'b2', 'b3'):
            assert torch.equal(f[name], pk['scan'][name])
        # an in-place weight change: both packs are rebuilt from the new parameter version
        with torch.no_grad():
            m.entropy_parameters[2].weight.mul_(1.5)
            m.context_prediction.weight.add_(0.25)
        pk2 = m._packed()
        assert pk2 is not pk and 'scan_f32' not in pk2
        f2 = m._scan_weights()
        want = _expected_pack(m)
        for name in ('wc', 'w1', 'w2', 'w3'):
            assert torch.equal(f2[name], want[name]), name
        assert not torch.equal(f2['w2'], f['w2']) and not torch.equal(f2['wc'], f['wc'])
        # the masked taps stay zero whatever the parameter holds there
        assert torch.equal(f2['wc'] != 0, want['wc'] != 0) and f2['wc'].shape[0] == 12 * m.M


# ---- the operating point is conclusive ----------------------------------------------------------- #
def test_float64_oracle_reproduces_the_f32_oracle_bytes():
    """Measured for seeds 0, 1, 2: 4 of 4 images, 37 - 38 distinct indexes."""
    ref, x, o = RM.world()
    assert abs(o['y'].std().item() - 4.0) < 1e-3 and abs(o['z'].std().item() - 3.0) < 1e-3
    assert abs(o['params'].std().item() - 2.0) < 1e-3
    assert tuple(o['y'].shape) == (4, RM.M_CH, 4, 8) and tuple(o['z'].shape) == (4, RM.N_CH, 1, 2)
    assert ref.entropy_parameters[0].out_channels == 133 and ref.entropy_parameters[2].out_channels == 106
    o64 = RM.chain(copy.deepcopy(ref).double(), x)
    same = RM.identical_images(o64, o)
    strings = [a == b for a, b in zip(o64['strings'], o['strings'])]
    n_idx = len(torch.unique(o['idx']))
    print('float64 oracle: integers of {} of {} images, strings of {}; {} distinct indexes; largest |symbol| {}'.format(
        sum(same), len(same), sum(strings), n_idx, int(o['y_sym'].abs().max())))
    assert sum(s and t for s, t in zip(same, strings)) >= 3
    assert all(t for s, t in zip(same, strings) if s)          # equal integers code to equal bytes
    assert n_idx >= 30
