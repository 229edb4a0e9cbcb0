"""The f32-grade codec modes of the neural input compression models (compression.py: `set_encoder_precision` on FactorizedPrior,
ScaleHyperprior, MeanScaleHyperprior) without a device: the interface, and the reference-alone conditions that
tests/test_gpu_precise_gdn2.py and tests/test_gpu_input_modes.py lean on, computed here on the CPU.

The conditions: (1) the CPU reference of the integer GDN cases -- sqrt and division in f64, rounded once -- is the correctly rounded
f32 result on every test value (so the zero-tolerance GPU test pins the device's sqrt and division to IEEE results, not to a CPU
quirk; torch's own f32 sqrt has one); (2) at the tests' operating point
(tests/ref_split_input.py) the share of symbols / indexes within delta = max(4e-6, 3 e_R) max|ref| of a rounding tie or a
scale-table boundary stays below the caps the GPU test sets, and the restatements code enough whole images to the oracle's
integers for the end-to-end test to be conclusive."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_split_input as ri  # noqa: E402

MODES = ('bf16', 'f32', 'bf16x3', 'bf16x6')
ZOO = {'FactorizedPrior': 'bmshj2018_factorized', 'ScaleHyperprior': 'bmshj2018_hyperprior', 'MeanScaleHyperprior': 'mbt2018_mean'}
PRECISE = {'f32': 'f64', 'bf16x3': 2, 'bf16x6': 3}
FLOOR = 4e-6
CAP_SYMBOLS = {'f32': 1e-3, 'bf16x6': 1e-3, 'bf16x3': 2e-3}
CAP_INDEXES = {'f32': 2e-3, 'bf16x6': 2e-3, 'bf16x3': 4e-3}


# ---- the interface ------------------------------------------------------------------------------ #
@pytest.mark.parametrize('name', list(ZOO))
def test_switch(S, name):
    m = S.COMPRESSION_MODEL_CLASS_DICT[name](16, 24)
    assert m.encoder_precision == 'bf16' and m._precise_ns() is None
    for mode, ns in zip(MODES, (None, 0, 2, 3)):
        assert m.set_encoder_precision(mode) is m
        assert m.encoder_precision == mode and m._precise_ns() == ns
    with pytest.raises(ValueError, match="encoder precision must be 'bf16', 'f32', 'bf16x3' or 'bf16x6'"):
        m.set_encoder_precision('fp16')
    assert m.encoder_precision == 'bf16x6'          # a refused name changes nothing
    assert S.COMPRESSION_MODEL_CLASS_DICT[name](16, 24, encoder_precision='bf16x3').encoder_precision == 'bf16x3'
    with pytest.raises(ValueError):
        S.COMPRESSION_MODEL_CLASS_DICT[name](16, 24, encoder_precision='f16')


@pytest.mark.parametrize('name', list(ZOO))
def test_config_kwarg_selects_the_mode(S, name):
    cfg = {'key': ZOO[name], 'kwargs': {'quality': 1, 'encoder_precision': 'f32'}, 'update': False}
    m = S.get_compression_model(cfg, torch.device('cpu'))
    assert type(m).__name__ == name and m.encoder_precision == 'f32'
    # the reference's own configs (no such key) load unchanged
    m = S.get_compression_model({'key': ZOO[name], 'kwargs': {'quality': 1}, 'update': False}, torch.device('cpu'))
    assert m.encoder_precision == 'bf16'
    # the mode is no parameter or buffer: state dicts are what they were
    assert not any('precision' in k for k in m.state_dict())


def test_mbt2018_refuses_precise_modes(S):
    m = S.COMPRESSION_MODEL_FUNC_DICT['mbt2018'](quality=1)
    assert m.encoder_precision == 'bf16' and m.set_encoder_precision('bf16') is m
    for mode in MODES[1:]:
        with pytest.raises(S.hip.Sc2Error, match='context scan'):
            m.set_encoder_precision(mode)
        assert m.encoder_precision == 'bf16'
        with pytest.raises(S.hip.Sc2Error):
            S.COMPRESSION_MODEL_FUNC_DICT['mbt2018'](quality=1, encoder_precision=mode)
    with pytest.raises(ValueError):
        m.set_encoder_precision('f64')


def test_walker_and_gdn_interface(S):
    from sc2bench_amd import entropy
    assert callable(entropy.run_hip_transform_precise)
    assert callable(S.GDN.forward_nhwc_precise) and S.GDN._precise_ops == (S.hip.AOP_SQUARE, S.hip.EPI_GDN2, S.hip.EPI_IGDN2)
    # geometry of g_a / g_s at the test shape: the widest map sizes the batch slices
    m = S.COMPRESSION_MODEL_CLASS_DICT['FactorizedPrior'](ri.N_CH, ri.M_CH)
    maps = entropy._precise_geometry(list(m.g_a), (4, 128, 192, 4))
    assert maps[1] == (4, 64, 96, 128) and maps[-1] == (4, 8, 12, 192)
    maps = entropy._precise_geometry(list(m.g_s), (4, 8, 12, 192))
    assert maps[-1] == (4, 128, 192, 3)


# ---- condition 1: the CPU reference of the integer GDN cases is correctly rounded ---------------- #
def _midpoints(t):
    """f64 midpoints between every f32 value and its two neighbours (25 significant bits: exact)."""
    lo = torch.nextafter(t, torch.full_like(t, -float('inf'))).double()
    hi = torch.nextafter(t, torch.full_like(t, float('inf'))).double()
    return (lo + t.double()) / 2, (hi + t.double()) / 2


@pytest.mark.parametrize('C', ri.GDN2_CHANNELS)
@pytest.mark.parametrize('pixels', ri.GDN2_PIXELS)
def test_cpu_sqrt_and_division_are_correctly_rounded(C, pixels):
    """The reference of tests/test_gpu_precise_gdn2.py takes sqrt and 1 / r in f64 and rounds once.  That this IS the correctly
    rounded f32 result is shown here without trusting any sqrt or division: r is the correctly rounded root of norm iff
    lo^2 <= norm <= hi^2 for the midpoints lo, hi to r's neighbours, q the correctly rounded 1 / r iff lo r <= 1 <= hi r; these
    products have at most 50 bits and are exact in f64.  torch's f32 division agrees on every value; torch's f32 sqrt does not on a
    CPU with AVX-512 (0.6 % of 1..4e6, among them 267 and 999), which is why the reference does not use it -- counted, not asserted."""
    x, gamma, beta, norm = ri.gdn2_int_case(C, pixels)
    r = torch.sqrt(norm.double()).float()
    lo, hi = _midpoints(r)
    assert bool((lo * lo <= norm.double()).all()) and bool((norm.double() <= hi * hi).all())
    q = (1.0 / r.double()).float()
    lo, hi = _midpoints(q)
    assert bool((lo * r.double() <= 1.0).all()) and bool((1.0 <= hi * r.double()).all())
    assert torch.equal(1.0 / r, q)                                     # torch's f32 division: correctly rounded
    print('C {} pixels {}: torch.sqrt (f32) differs from the correctly rounded root on {} of {} values'.format(
        C, pixels, int((torch.sqrt(norm) != r).sum()), norm.numel()))
    assert torch.equal(ri.gdn2_int_expected(x, norm, False), (x.double() * q.double()).float())
    assert torch.equal(ri.gdn2_int_expected(x, norm, True), (x.double() * r.double()).float())
    # the cases are no trivial ones: the roots are inexact
    assert (r.double() * r.double() != norm.double()).any() or norm.numel() < 200


# ---- condition 2: exclusion caps and identical-image counts ------------------------------------- #
_WORLDS = {}


def _world(name):
    if name not in _WORLDS:
        ref = ri.build(name)
        x = ri.images()
        _WORLDS[name] = (ref, x, ri.stages(ref, x, 'f32'))
    return _WORLDS[name]


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def _tie_distance(t):
    return ((t - torch.floor(t)) - 0.5).abs()


def left_out_shares(ref, o, rest):
    """-> dict(what -> share of elements within delta of a tie / boundary) for the restatement `rest` (stage-wise) of oracle `o`."""
    eb = ref.entropy_bottleneck
    delta = {k: max(FLOOR, 3 * _rel(rest[k], o[k])) * o[k].abs().max().item() for k in ('y', 'z', 'params') if k in o}
    out = {}
    if ri.has_hyper(ref):
        mu = o['means'] if o['means'] is not None else 0.0
        out['y symbols'] = 1.0 - (_tie_distance(o['y'] - mu) > delta['y']).float().mean().item()
        out['z symbols'] = 1.0 - (_tie_distance(o['z'] - ri.medians(eb, o['z'])) > delta['z']).float().mean().item()
        near = torch.zeros_like(o['scales'], dtype=torch.bool)
        for t in ref.gaussian_conditional.scale_table[:-1]:
            near |= (o['scales'] - t).abs() <= delta['params']
        out['indexes'] = near.float().mean().item()
    else:
        out['y symbols'] = 1.0 - (_tie_distance(o['y'] - ri.medians(eb, o['y'])) > delta['y']).float().mean().item()
    return out


@pytest.mark.parametrize('name', ri.NAMES)
@pytest.mark.parametrize('mode', list(PRECISE))
def test_operating_point_is_conclusive(name, mode):
    ref, x, o = _world(name)
    assert abs(o['y'].std().item() - 4.0) < 1e-3
    if ri.has_hyper(ref):
        assert abs(o['z'].std().item() - 3.0) < 1e-3 and abs(o['params'].std().item() - 2.0) < 1e-3
        assert tuple(o['y'].shape[-2:]) == (8, 12) and tuple(o['z'].shape[-2:]) == (2, 3)
    stage_wise = ri.stages(ref, x, PRECISE[mode], inputs=o)
    for what, share in left_out_shares(ref, o, stage_wise).items():
        cap = (CAP_INDEXES if what == 'indexes' else CAP_SYMBOLS)[mode]
        print('{} {} {}: {:.2e} of the elements within delta of a tie / boundary (cap {:.0e})'.format(name, mode, what, share, cap))
        assert share <= cap
    end_to_end = ri.stages(ref, x, PRECISE[mode], y=stage_wise['y'])
    n = sum(ri.identical_images(ri.int_tensors(end_to_end), ri.int_tensors(o)))
    print('{} {}: the restatement codes {} of {} images to the oracle\'s integers'.format(name, mode, n, ri.N_IMAGES))
    if mode in ('f32', 'bf16x6'):
        assert n >= 2
