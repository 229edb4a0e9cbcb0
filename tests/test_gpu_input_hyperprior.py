"""-m gpu: the hyperprior and joint-autoregressive input codecs (bmshj2018_hyperprior, mbt2018_mean, mbt2018) on the HIP
library against the f32 restatement (tests/ref_input_hyperprior.py) with seeded random weights.

Integer work is exact: byte streams given the device's symbols and indexes, y_hat of the decoder given the encoder's (the
serial scan of csrc/ar_context.hip runs the same step code in both directions).  Floating point: bf16 operands through a
stack of layers vs f32, as tests/test_gpu_input_compression.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_input_hyperprior as RH  # noqa: E402

BF16_REL_L2 = 1.5e-2
SPREAD = 8.0      # g_a's last weights scaled so the latent covers several symbols


def rel(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-12)).item()


_MODELS = {}


def _pair(S, dev, name, quality, seed=0):
    key = (name, quality, seed)
    if key not in _MODELS:
        torch.manual_seed(seed)
        r = RH.build(name, quality).eval()
        with torch.no_grad():
            r.g_a[6].weight.mul_(SPREAD)
        r.update()
        m = S.COMPRESSION_MODEL_FUNC_DICT[name](quality=quality)
        m.load_state_dict({k: v.clone() for k, v in r.state_dict().items()})
        m.eval().to(dev)
        _MODELS[key] = (m, r)
    return _MODELS[key]


def _image(B, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, size, size, generator=g)
    # smooth the noise a little so the codecs see image-like statistics
    return torch.nn.functional.avg_pool2d(x, 3, 1, 1)


def _bits(lik):
    return float((-torch.log2(lik.float().cpu().clamp_min(1e-30))).sum())


@pytest.mark.parametrize('name,quality', [('bmshj2018_hyperprior', 1), ('mbt2018_mean', 1), ('mbt2018', 8)])
def test_forward_matches_restatement(S, dev, name, quality):
    m, r = _pair(S, dev, name, quality)
    x = _image(2, 64)
    with torch.no_grad():
        out = m(x.to(dev))
        ref = r(x)
    # with means, y_hat = round(y - mean) + mean: bf16 means flip a few roundings, so x_hat is held to the full chain's bound
    assert rel(out['x_hat'], ref['x_hat']) < (BF16_REL_L2 if name == 'bmshj2018_hyperprior' else 3e-2)
    for k in ('y', 'z'):
        assert out['likelihoods'][k].shape == ref['likelihoods'][k].shape
        b, rb = _bits(out['likelihoods'][k]), _bits(ref['likelihoods'][k])
        assert abs(b - rb) <= 0.02 * rb + 16, (k, b, rb)


@pytest.mark.parametrize('name', ['bmshj2018_hyperprior', 'mbt2018_mean'])
def test_hyperprior_compression_bytes_and_round_trip(S, dev, name):
    from oracle import rans as oracle_rans
    m, r = _pair(S, dev, name, 1)
    x = _image(3, 64, seed=1)
    gc = m.gaussian_conditional
    with torch.no_grad():
        obj = m.compress(x.to(dev))
        y = m.analysis(x.to(dev))
        z_hat_nhwc = m._z_hat_nhwc(obj['strings'][1], obj['shape'])
        scales, means = m._gaussian(m.hyper_synthesis(z_hat_nhwc))
        idx = gc.build_indexes(scales)
        sym = gc.quantize(y, 'symbols', means)
        tabs = (gc._quantized_cdf.cpu().numpy(), gc._cdf_length.cpu().numpy(), gc._offset.cpu().numpy())
        for i in range(3):
            assert obj['strings'][0][i] == oracle_rans.encode_with_indexes(sym[i].cpu().reshape(-1), idx[i].cpu().reshape(-1),
                                                                           *tabs)
        z = m.hyper_analysis(y)
        ref_z = r.entropy_bottleneck.compress(z.cpu())
        assert obj['strings'][1] == ref_z          # z bytes: the oracle's coder on the device's z
        y_dec = gc.decompress(obj['strings'][0], idx, means=means)
        assert torch.equal(y_dec, gc.dequantize(sym, means))
        # symbols against the f32 restatement
        ry = r.g_a(x)
        rz_hat = r.entropy_bottleneck.decompress(r.entropy_bottleneck.compress(r.h_a(r._hyper_in(ry))), obj['shape'])
        _, rmeans = r._gaussian(r.h_s(rz_hat))
        rsym = r.gaussian_conditional.quantize(ry, 'symbols', rmeans)
        agree = (rsym == sym.cpu()).float().mean().item()
        assert agree >= 0.995, agree
        out = m.decompress(**obj)
    assert out['x_hat'].shape == x.shape


def _scan_ref_params(r, m, z_strings, shape):
    with torch.no_grad():
        z_hat = m.entropy_bottleneck.decompress(z_strings, shape)
        return r.h_s(z_hat.cpu())


@pytest.mark.parametrize('size,B', [(64, 2), (256, 4)])
def test_mbt2018_teacher_forced_step(S, dev, size, B):
    """Given the scan's own y_hat, each step's scales / means equal the restatement's parallel context path."""
    m, r = _pair(S, dev, 'mbt2018', 8)
    x = _image(B, size, seed=2)
    M = m.M
    with torch.no_grad():
        H = W = size // 16
        gp = torch.empty((B, H * W, 2 * M), dtype=torch.float32, device=dev)
        enc = m.compress_device(x.to(dev), gaussian_params=gp)
        y_hat = enc['y_hat_pad'][:, 2:, 2:-2].permute(0, 3, 1, 2).contiguous().cpu()
        params = _scan_ref_params(r, m, enc['z_strings'], enc['shape'])
        ref = r.gaussian_params(params, y_hat)                           # [B, 2M, H, W]
    got = gp.cpu().reshape(B, H, W, 2 * M).permute(0, 3, 1, 2)
    assert rel(got[:, :M], ref[:, :M]) < BF16_REL_L2
    assert rel(got[:, M:], ref[:, M:]) < BF16_REL_L2
    ref_idx = r.gaussian_conditional.build_indexes(ref[:, :M]).permute(0, 2, 3, 1).reshape(B, -1)
    agree = (ref_idx == enc['indexes'].cpu()).float().mean().item()
    assert agree >= 0.99, agree
    # y_hat = symbol + mean of the step, the symbol = round(y - mean)
    sym = enc['symbols'].cpu().reshape(B, H, W, M).permute(0, 3, 1, 2)
    assert torch.equal(y_hat, sym.float() + got[:, M:])
    assert torch.equal(sym, torch.round(enc['y'].cpu() - got[:, M:]).int())


@pytest.mark.parametrize('size,B', [(64, 3), (256, 2)])
def test_mbt2018_round_trip_is_bit_exact(S, dev, size, B):
    from oracle import rans as oracle_rans
    m, _ = _pair(S, dev, 'mbt2018', 8)
    gc = m.gaussian_conditional
    x = _image(B, size, seed=3)
    with torch.no_grad():
        enc = m.compress_device(x.to(dev))
        obj = m.compress(x.to(dev))
        y_pad, y_hat, sym = m.decompress_device(obj['strings'], obj['shape'])
        assert torch.equal(y_pad, enc['y_hat_pad'])
        assert torch.equal(sym, enc['symbols'])
        y_pad3, y_hat3, _ = m.decompress_device(obj['strings'], obj['shape'], chunks=3)   # the scan resumed twice
        assert torch.equal(y_pad3, y_pad) and torch.equal(y_hat3, y_hat)
        assert torch.equal(y_hat.float(), y_pad[:, 2:, 2:-2].to(torch.bfloat16).float())
        out = m.decompress(**obj)
        assert torch.equal(out['x_hat'], m.synthesis_nhwc(y_hat).clamp_(0, 1))
    tabs = (gc._quantized_cdf.cpu().numpy(), gc._cdf_length.cpu().numpy(), gc._offset.cpu().numpy())
    for i in range(B):
        s, ix = enc['symbols'][i].cpu().numpy(), enc['indexes'][i].cpu().numpy()
        assert obj['strings'][0][i] == oracle_rans.encode_with_indexes(s, ix, *tabs)
        assert np.array_equal(oracle_rans.decode_with_indexes(obj['strings'][0][i], ix, *tabs), s)


def test_resumable_decoder_kernel(S, dev):
    """sc2_rans_decode_resume in three pieces returns the oracle's symbols and ends each stream cleanly."""
    from oracle import rans as oracle_rans
    m, _ = _pair(S, dev, 'mbt2018', 8)
    gc = m.gaussian_conditional
    tabs = (gc._quantized_cdf.cpu().numpy(), gc._cdf_length.cpu().numpy(), gc._offset.cpu().numpy())
    g = torch.Generator().manual_seed(4)
    n = 3000
    idx = torch.randint(0, 64, (5, n), generator=g, dtype=torch.int32)
    sym = (torch.randn(5, n, generator=g) * (idx.float() + 1) * 2).round().int()
    sym[0, :40] = 100000     # escapes
    strings = [oracle_rans.encode_with_indexes(sym[i].numpy(), idx[i].numpy(), *tabs) for i in range(5)]
    buf, off, nb = gc.pack_strings(strings, dev)
    cdf, cdf_len, offset = gc._tables()
    idx_d = idx.to(dev)
    cuts = [0, 7, 1700, n]
    state, parts = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s, state = S.hip.rans_decode_resume(buf, off, nb, idx_d[:, a:b].contiguous(), cdf, cdf_len.int(), offset.int(),
                                            state=state, last=b == n)
        parts.append(s)
    assert torch.equal(torch.cat(parts, 1).cpu(), sym)
    assert int(state[2].abs().max()) == 0


def test_mbt2018_batch_invariance(S, dev):
    m, _ = _pair(S, dev, 'mbt2018', 8)
    x = _image(5, 64, seed=5)
    with torch.no_grad():
        alone = m.compress(x[3:4].to(dev))
        batch = m.compress(x.to(dev))
        first = m.compress(torch.cat([x[3:4], x[:3], x[4:]]).to(dev))
        assert batch['strings'][0][3] == alone['strings'][0][0] == first['strings'][0][0]
        assert batch['strings'][1][3] == alone['strings'][1][0] == first['strings'][1][0]
        # decode the image in a mixed batch: the same y_hat as alone
        _, y_alone, _ = m.decompress_device(alone['strings'], alone['shape'])
        mixed = [batch['strings'][0][i] for i in (0, 3, 1)], [batch['strings'][1][i] for i in (0, 3, 1)]
        _, y_mixed, _ = m.decompress_device([mixed[0], mixed[1]], batch['shape'])
        assert torch.equal(y_mixed[1], y_alone[0])


def test_mbt2018_hostile_streams_raise(S, dev):
    m, _ = _pair(S, dev, 'mbt2018', 8)
    x = _image(2, 64, seed=6)
    with torch.no_grad():
        obj = m.compress(x.to(dev))
        ys = obj['strings'][0]
        truncated = [ys[0][:len(ys[0]) // 2], ys[1]]
        with pytest.raises(ValueError):
            m.decompress([truncated, obj['strings'][1]], obj['shape'])
        rng = np.random.default_rng(7)
        garbage = [rng.integers(0, 256, len(ys[0]), dtype=np.uint8).tobytes(), ys[1]]
        with pytest.raises(ValueError):
            m.decompress([garbage, obj['strings'][1]], obj['shape'])
        # the device is fine afterwards
        out = m.decompress(**obj)
    assert torch.isfinite(out['x_hat']).all()


@pytest.mark.parametrize('name,quality', [('bmshj2018_hyperprior', 1), ('mbt2018_mean', 1), ('mbt2018', 8)])
def test_full_chain_against_restatement(S, dev, name, quality):
    m, r = _pair(S, dev, name, quality)
    x = _image(2, 64, seed=8)
    with torch.no_grad():
        obj = m.compress(x.to(dev))
        out = m.decompress(**obj)
        robj = r.compress(x)
        rout = r.decompress(**robj)

    def nbytes(o):
        return sum(len(s) for lst in o['strings'] for s in lst)
    assert abs(nbytes(obj) - nbytes(robj)) <= 0.02 * nbytes(robj) + 8, (nbytes(obj), nbytes(robj))
    assert rel(out['x_hat'], rout['x_hat']) <= 3e-2


def test_neural_input_compression_classifier_with_mbt2018(S, dev):
    from sc2bench_amd import transforms as T
    from sc2bench_amd.resnet import resnet50
    m, _ = _pair(S, dev, 'mbt2018', 8)
    torch.manual_seed(5)
    clf = resnet50(num_classes=10).eval()
    post = T.Compose([T.CenterCrop([64, 64])])
    wrapped = S.NeuralInputCompressionClassifier(
        clf, pre_transform=T.AdaptivePad(fill=0, factor=64), compression_model=m, post_transform=post,
        analysis_config={'analyzes_after_compress': True, 'analyzer_configs': [{'key': 'FileSizeAnalyzer', 'kwargs': {'unit': 'KB'}}]})
    wrapped.eval().to(dev)
    wrapped.activate_analysis()
    x = _image(2, 56, seed=9)
    with torch.no_grad():
        out = wrapped(x.to(dev))
        obj = m.compress(T.AdaptivePad(fill=0, factor=64)(x.to(dev)))
    assert out.shape == (2, 10) and torch.isfinite(out.float()).all()
    sizes = wrapped.analyzers[0].file_size_list
    import pickle
    assert len(sizes) == 1 and sizes[0] > 0
    assert len(obj['strings']) == 2 and sizes[0] * 1024 >= sum(len(s) for s in obj['strings'][0])
    assert sizes[0] == pytest.approx(sys.getsizeof(pickle.dumps(obj)) / 1024, rel=0.05)


@pytest.mark.parametrize('name,stem', [('bmshj2018_hyperprior', 'bmshj2018-hyperprior'), ('mbt2018_mean', 'mbt2018-mean'),
                                       ('mbt2018', 'mbt2018')])
def test_pretrained_weights_from_local_dir(S, dev, tmp_path, monkeypatch, name, stem):
    torch.manual_seed(11)
    r = RH.build(name, 1)
    r.update()
    sd = {k: v.clone() for k, v in r.state_dict().items()}
    for i in range(4):       # CompressAI <= 1.1 key names of the entropy bottleneck
        sd['entropy_bottleneck._matrix{}'.format(i)] = sd.pop('entropy_bottleneck.matrices.{}'.format(i))
    torch.save(sd, str(tmp_path / '{}-mse-1.pth'.format(stem)))
    monkeypatch.setenv('SC2_PRETRAINED_DIR', str(tmp_path))
    m = S.COMPRESSION_MODEL_FUNC_DICT[name](quality=1, pretrained=True)
    assert torch.equal(m.entropy_bottleneck.matrices[0], r.entropy_bottleneck.matrices[0])
    assert torch.equal(m.g_a[0].weight, r.g_a[0].weight)
    m.to(dev).eval()
    with torch.no_grad():
        obj = m.compress(_image(1, 64).to(dev))
        assert m.decompress(**obj)['x_hat'].shape == (1, 3, 64, 64)
