"""CPU: the hyperprior and joint-autoregressive input codecs (bmshj2018_hyperprior, mbt2018_mean, mbt2018) -- registration,
quality tables, parameter / buffer names against the f32 restatement (tests/ref_input_hyperprior.py), the context mask, the
restatement's own serial round trip, and the reference's configs building their compression models."""
import glob
import os
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_input_hyperprior as RH  # noqa: E402

REF = '/root/reference/configs'
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason='reference tree not present')
ZOO = ('bmshj2018_hyperprior', 'mbt2018_mean', 'mbt2018')


def test_zoo_functions_registered(S):
    for name in ZOO:
        assert name in S.COMPRESSION_MODEL_FUNC_DICT
    for cls in ('ScaleHyperprior', 'MeanScaleHyperprior', 'JointAutoregressiveHierarchicalPriors'):
        assert cls in S.COMPRESSION_MODEL_CLASS_DICT


def test_quality_tables(S):
    from sc2bench_amd import compression as C
    expect = {'bmshj2018_hyperprior': (C.ScaleHyperprior, [(128, 192)] * 5 + [(192, 320)] * 3),
              'mbt2018_mean': (C.MeanScaleHyperprior, [(128, 192)] * 4 + [(192, 320)] * 4),
              'mbt2018': (C.JointAutoregressiveHierarchicalPriors, [(192, 192)] * 4 + [(192, 320)] * 4)}
    for name, (cls, nm) in expect.items():
        for q in (1, 4, 5, 8):
            m = S.COMPRESSION_MODEL_FUNC_DICT[name](quality=q)
            assert type(m) is cls and (m.N, m.M) == nm[q - 1], (name, q)
            assert RH.ZOO[name][1][q] == nm[q - 1]
        for bad in (0, 9):
            with pytest.raises(ValueError):
                S.COMPRESSION_MODEL_FUNC_DICT[name](quality=bad)
        with pytest.raises(ValueError):
            S.COMPRESSION_MODEL_FUNC_DICT[name](quality=1, metric='psnr')


@pytest.mark.parametrize('name', ZOO)
def test_state_dict_matches_restatement(S, name):
    torch.manual_seed(0)
    m = S.COMPRESSION_MODEL_FUNC_DICT[name](quality=1)
    r = RH.build(name, 1)
    sd, rsd = m.state_dict(), r.state_dict()
    assert set(sd) == set(rsd)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(rsd[k].shape), k
    for k in ('gaussian_conditional._quantized_cdf', 'gaussian_conditional._offset', 'gaussian_conditional._cdf_length',
              'gaussian_conditional.scale_table', 'gaussian_conditional.scale_bound'):
        assert k in sd
    if name == 'mbt2018':
        assert 'context_prediction.mask' in sd
        assert torch.equal(sd['context_prediction.mask'], rsd['context_prediction.mask'])


def test_context_mask_has_the_12_causal_taps(S):
    m = S.mbt2018(quality=1)
    mask = m.context_prediction.mask
    assert tuple(mask.shape) == (384, 192, 5, 5)
    tap = mask[0, 0]
    assert int(tap.sum().item()) == 12
    keep = [(ky, kx) for ky in range(2) for kx in range(5)] + [(2, 0), (2, 1)]
    for ky in range(5):
        for kx in range(5):
            assert tap[ky, kx].item() == (1.0 if (ky, kx) in keep else 0.0)
    assert torch.equal(mask, tap.expand_as(mask))


def test_load_state_dict_resizes_gaussian_buffers(S):
    torch.manual_seed(0)
    r = RH.build('mbt2018_mean', 1)
    r.update()
    m = S.mbt2018_mean(quality=1)
    sd = {k: v.clone() for k, v in r.state_dict().items()}
    m.load_state_dict(sd)
    assert torch.equal(m.gaussian_conditional._quantized_cdf, r.gaussian_conditional._quantized_cdf)
    assert torch.equal(m.gaussian_conditional.scale_table, r.gaussian_conditional.scale_table)
    m2 = type(m).from_state_dict({k: v.clone() for k, v in r.state_dict().items()})
    assert (m2.N, m2.M) == (128, 192)


def _small_mbt(seed=0, N=16, M=24):
    torch.manual_seed(seed)
    r = RH.JointAutoregressiveHierarchicalPriors(N, M).eval()
    with torch.no_grad():
        r.g_a[6].weight.mul_(6.0)   # spread the latent over several symbols
    r.update()
    return r


def test_restatement_serial_round_trip():
    r = _small_mbt()
    x = torch.rand(2, 3, 64, 64)
    with torch.no_grad():
        y = r.g_a(x)
        z_hat = r.entropy_bottleneck.decompress(r.entropy_bottleneck.compress(r.h_a(y)), (1, 1))
        params = r.h_s(z_hat)
        strings, sym, idx, y_hat = r.compress_ar(y, params)
        assert sym.shape == (2, 16 * 24) and int(sym.abs().max()) > 0
        y_dec = r.decompress_ar(strings, params)
    assert torch.equal(y_dec, y_hat)
    # the serial y_hat is what the parallel context path sees: its means are the scan's means
    cdf, cdf_len, offsets = r._tables()
    from oracle import rans as oracle_rans
    assert list(oracle_rans.decode_with_indexes(strings[0], idx[0], cdf, cdf_len, offsets)) == sym[0].tolist()
    with torch.no_grad():
        obj = r.compress(x)
        out = r.decompress(**obj)
    assert out['x_hat'].shape == x.shape


def test_restatement_round_trip_with_escapes():
    """Symbols beyond the Gaussian table's range are coded through the bypass escapes and come back."""
    r = _small_mbt(seed=1)
    y = torch.randn(1, 24, 4, 4) * 300.0
    params = torch.randn(1, 48, 4, 4)
    with torch.no_grad():
        strings, sym, _, y_hat = r.compress_ar(y, params)
        assert int(sym.abs().max()) > 100
        assert torch.equal(r.decompress_ar(strings, params), y_hat)


@needs_ref
def test_reference_configs_build_their_compression_models(S):
    paths = []
    for stem in ('scale_hyperprior', 'mean_scale_hyperprior', 'joint_autoregressive_hierarchical_prior'):
        paths += sorted(glob.glob(os.path.join(REF, '*', 'input_compression', stem + '-*.yaml')))
    assert len(paths) == 16
    kinds = {'bmshj2018_hyperprior': S.ScaleHyperprior, 'mbt2018_mean': S.MeanScaleHyperprior,
             'mbt2018': S.JointAutoregressiveHierarchicalPriors}
    from sc2bench_amd import config
    for p in paths:
        cfg = config.load_yaml_file(p)
        found = []

        def walk(node):
            if isinstance(node, dict):
                if 'compression_model' in node and isinstance(node['compression_model'], dict):
                    found.append(node['compression_model'])
                for v in node.values():
                    walk(v)
            elif isinstance(node, list):
                for v in node:
                    walk(v)
        walk(cfg['models'])
        assert found, p
        for cm in found:
            key = cm['key']
            assert key in kinds, (p, key)
            if p.endswith('resnet50.yaml'):
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    model = S.get_compression_model(dict(cm, update=False), 'cpu')
                assert type(model) is kinds[key], p
                if key == 'mbt2018':
                    assert (model.N, model.M) == (192, 320)
            else:
                kwargs = dict(cm.get('kwargs') or {})
                kwargs['pretrained'] = False
                assert type(S.COMPRESSION_MODEL_FUNC_DICT[key](**kwargs)) is kinds[key], p
