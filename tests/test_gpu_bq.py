"""GPU: the CR+BQ baseline end to end -- `custom_resnet50` (larger_resnet_bottleneck + SimpleQuantizer / SimpleDequantizer +
layer3 .. fc) in eval mode on the library's kernels against the f32 restatement on the CPU (tests/ref_bq.py).

Fences: the project's bf16-against-f32 one, max |err| <= 0.03 s + 0.03 with s = max |reference| (tests/test_gpu_bottleneck.py),
wherever both sides see the same bytes; 0.08 s + 0.08 end to end, where bf16 arithmetic in front of the quantizer may flip codes.
The codes themselves are held to the bit: quantizing the device's own latent with the restatement must reproduce them."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_bq as rb  # noqa: E402

pytestmark = pytest.mark.gpu

INPUTS = [(2, 3, 64, 64), (1, 3, 72, 56)]
LATENT_HW = {(64, 64): (9, 9), (72, 56): (10, 8)}


def _fence(got, want, rel=0.03):
    s = want.abs().max().item()
    err = (got.float().cpu() - want).abs().max().item()
    print('max err {:.5f}  fence {:.5f}  (s = {:.4f})'.format(err, rel * s + rel, s))
    assert err <= rel * s + rel, 'max err {} > {} * {} + {}'.format(err, rel, s, rel)


class _Capture(object):
    def __init__(self):
        self.seen = []

    def analyze(self, obj):
        self.seen.append(obj)

    def clear(self):
        del self.seen[:]


def _build(S, dev, channels, idx, bits=8, per_sample=False, dtype='bf16'):
    """(model on the device, f32 restatement of its bottleneck, f32 copy of its task head) with shared weights"""
    from sc2bench_amd.transforms import Compose
    torch.manual_seed(100 * channels + idx)
    quantizer = S.SimpleQuantizer(bits, per_sample=per_sample) if per_sample else S.SimpleQuantizer(bits)
    m = S.custom_resnet50(bottleneck_channel=channels, bottleneck_idx=idx, compressor=Compose([quantizer]),
                          decompressor=Compose([S.SimpleDequantizer(bits)]), num_classes=1000,
                          analysis_config={'analyzes_after_compress': True,
                                           'analyzer_configs': [{'key': 'FileSizeAnalyzer', 'kwargs': {'unit': 'KB'}}]})
    rb.randomise_norms(m, seed=channels + idx)
    ref = rb.Bottleneck(channels, idx, quantized=bits == 8)
    ref.load_state_dict(m.bottleneck_layer.state_dict())
    tail = copy.deepcopy(torch.nn.Sequential(m.layer3, m.layer4, m.avgpool, torch.nn.Flatten(1), m.fc))
    m.eval().to(dev)
    m.set_compute_dtype(dtype)
    return m, ref.eval(), tail.eval()


_MODELS = {}


def _model(S, dev, channels, idx):
    key = (channels, idx)
    if key not in _MODELS:
        _MODELS[key] = _build(S, dev, channels, idx)
    return _MODELS[key]


@pytest.mark.parametrize('shape', INPUTS)
@pytest.mark.parametrize('idx', [7, 9])
@pytest.mark.parametrize('channels', [12, 3, 1])
def test_eval_forward_against_restatement(S, dev, channels, idx, shape):
    m, ref, tail = _model(S, dev, channels, idx)
    bl = m.bottleneck_layer
    x = torch.rand(shape, generator=torch.Generator().manual_seed(shape[2]))
    with torch.no_grad():
        enc = bl.encode(x.to(dev))
        latent = bl.analysis(x.to(dev))
        z = enc['z']
        assert set(enc) == {'z'} and isinstance(z, S.QuantizedTensor)
        assert z.tensor.is_cuda and z.tensor.dtype == torch.uint8
        assert z.tensor.shape == (shape[0], channels) + LATENT_HW[shape[2:]]
        assert z.scale.dim() == 0 and z.scale.is_cuda and isinstance(z.zero_point, int)
        # the codes are the restatement's, to the bit, on the device's own latent
        want = rb.quantize(latent.cpu())
        assert torch.equal(z.tensor.cpu(), want.tensor) and z.zero_point == want.zero_point
        assert z.scale.cpu().view(torch.int32).item() == want.scale.view(torch.int32).item()
        if idx == 9:
            assert z.zero_point == 0 and float(latent.min()) >= 0.0
        _fence(latent, ref.encoder(x))
        # the decoder on the device's own bytes
        on_bytes = ref.decode(rb.Quantized(z.tensor.cpu(), z.scale.cpu(), z.zero_point))
        dec = bl.decode(**enc)
        assert dec.dtype == torch.bfloat16 and dec.shape == on_bytes.shape and dec.permute(0, 2, 3, 1).is_contiguous()
        _fence(dec, on_bytes)
        logits = m(x.to(dev))
        assert logits.shape == (shape[0], 1000)
        _fence(logits, tail(on_bytes))
        _fence(logits, tail(ref(x)), rel=0.08)      # end to end against the pure-f32 path: includes quantization flips
    assert bl._bq_plan is not None and m._hip_head is not None, 'the eval forward must run the HIP bottleneck and the HIP head'


def test_f32_compute_dtype(S, dev):
    m, ref, tail = _build(S, dev, 12, 7, dtype='f32')
    x = torch.rand(INPUTS[0], generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        enc = m.bottleneck_layer.encode(x.to(dev))
        z = enc['z']
        dec = m.bottleneck_layer.decode(**enc)
        on_bytes = ref.decode(rb.Quantized(z.tensor.cpu(), z.scale.cpu(), z.zero_point))
        assert dec.dtype == torch.float32 and dec.is_contiguous() and dec.shape == on_bytes.shape
        _fence(dec, on_bytes)
        _fence(m(x.to(dev)), tail(on_bytes))


def test_sixteen_bits_round_trips_through_half(S, dev):
    m, ref, tail = _build(S, dev, 12, 7, bits=16)
    bl = m.bottleneck_layer
    x = torch.rand(INPUTS[0], generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        enc = bl.encode(x.to(dev))
        assert enc['z'].dtype == torch.float16 and torch.equal(enc['z'], bl.analysis(x.to(dev)).half())
        on_half = ref.decode(enc['z'].float().cpu())
        _fence(bl.decode(**enc), on_half)
        _fence(m(x.to(dev)), tail(on_half))


def test_per_sample_equals_each_image_alone(S, dev):
    m, ref, tail = _build(S, dev, 12, 7, per_sample=True)
    bl = m.bottleneck_layer
    spread = torch.tensor([1.0, 0.2]).reshape(2, 1, 1, 1)
    x = torch.rand(INPUTS[0], generator=torch.Generator().manual_seed(3)) * spread
    with torch.no_grad():
        latent = bl.analysis(x.to(dev))
        z = bl.encode(x.to(dev))['z']
        assert z.scale.shape == (2,) and z.zero_point.shape == (2,)
        dec = bl.decode(z)
        logits = m(x.to(dev))
        for i in range(2):
            alone = S.quantize_tensor(latent[i:i + 1])          # the reference's batch-size-1 evaluation of this image
            want = rb.quantize(latent[i:i + 1].cpu())
            assert torch.equal(z.tensor[i:i + 1], alone.tensor) and torch.equal(alone.tensor.cpu(), want.tensor)
            assert int(z.zero_point[i]) == alone.zero_point == want.zero_point
            assert z.scale[i].cpu().view(torch.int32).item() == want.scale.view(torch.int32).item()
            on_bytes = ref.decode(want)
            _fence(dec[i:i + 1], on_bytes)
            _fence(logits[i:i + 1], tail(on_bytes))
        assert float(z.scale[0]) != float(z.scale[1])


def test_analyzer_and_kernel_tags(S, dev):
    m, ref, tail = _model(S, dev, 12, 7)
    x = torch.rand(INPUTS[0], generator=torch.Generator().manual_seed(4)).to(dev)
    capture = _Capture()
    m.analyzers.append(capture)
    m.update()
    m.activate_analysis()
    try:
        with torch.no_grad():
            m(x)                # (first call: builds the folded weights)
            m.clear_analysis()
            with S.hip.KernelTimer() as timer:
                m(x)
        torch.cuda.synchronize()
    finally:
        m.deactivate_analysis()
        m.analyzers.remove(capture)
    assert len(capture.seen) == 1 and isinstance(capture.seen[0]['z'], S.QuantizedTensor)
    assert capture.seen[0]['z'].tensor.dtype == torch.uint8
    assert len(m.analyzers[0].file_size_list) == 1 and m.analyzers[0].file_size_list[0] > 12 * 81 * 2 / 1024
    counts = {}
    for tag, (count, _) in timer.summary().items():
        for part in tag.split('+'):         # (a fused pair of head layers carries both names)
            counts[part] = counts.get(part, 0) + count
    for tag in ('bq.quantize', 'bq.dequantize', 'bq.pool', 'bq.avgpool', 'bq.layout'):
        assert counts.get(tag) == 1, (tag, counts)
    convs = ['bq.stem', 'bq.conv_z', 'bq.dec0', 'bq.dec1', 'bq.dec2', 'bq.dec3', 'head.fc']
    for layer, blocks in ((3, 6), (4, 3)):
        for b in range(blocks):
            convs += ['head.{}.{}.c{}'.format(layer, b, c) for c in (1, 2, 3)]
        convs.append('head.{}.0.ds'.format(layer))
    for tag in convs:       # every layer ran as a tagged launch of the library: nothing fell back to torch ops
        assert counts.get(tag) == 1, (tag, counts)


def test_head_with_layer2_is_unchanged(S, dev):
    """the relaxed condition of SplittableResNet.head: a model that has layer2 takes the HIP head exactly as before"""
    torch.manual_seed(0)
    cfg = {'key': 'FPBasedResNetBottleneck', 'kwargs': {'num_bottleneck_channels': 24, 'num_target_channels': 256}}
    m = S.splittable_resnet(cfg, skips_avgpool=False, skips_fc=False, num_classes=1000)
    m.eval().to(dev)
    m.set_compute_dtype('bf16')
    x = torch.rand(1, 3, 64, 64).to(dev)
    with torch.no_grad(), S.hip.KernelTimer() as timer:
        out = m(x)
    torch.cuda.synchronize()
    assert out.shape == (1, 1000) and bool(torch.isfinite(out).all())
    assert m._hip_head is not None and len(m._hip_head.blocks) == 4 + 6 + 3
    tags = {part for tag in timer.summary() for part in tag.split('+')}
    assert 'head.2.0.c2' in tags and 'head.3.0.c1' in tags and 'head.4.2.c3' in tags and 'head.fc' in tags
