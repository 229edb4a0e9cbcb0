"""-m gpu: the task head's outputs, bit for bit.

The logits of a seeded bs-2 `HipHead` over layer2 .. fc on a 2 x 256 x 56 x 56 bf16 map (the model of
tests/test_gpu_conv1x1_w8.py::test_head_policy) and the input gradient of `FrozenStack` layer3 on 2 x 512 x 28 x 28 must hash to the
digests in tests/golden/head_bits.json, recorded on an MI355X before `head._Conv`'s dispatch was given one routing function: the same
kernels with the same arguments in the same order give the same bytes (recorded twice, in two processes, with equal digests).  Every
operand is made on the CPU from a seed, so the bytes that reach the device do not depend on the machine.  A change that moves a layer
to another kernel, or changes a kernel's arithmetic, moves these digests ON PURPOSE and records them anew
(`python tests/test_gpu_head_bits.py` prints them); there is no tolerance to widen.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'head_bits.json')
BF16 = torch.bfloat16


def _randomise_bn(module):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)


def _sha(t):
    t = t.detach().cpu().contiguous()
    return '{} {} {}'.format(str(t.dtype).replace('torch.', ''), 'x'.join(str(v) for v in t.shape),
                             hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())


def head_logits(S, dev):
    torch.manual_seed(5)
    cfg = {'key': 'FPBasedResNetBottleneck', 'kwargs': {'num_bottleneck_channels': 24, 'num_target_channels': 256}}
    model = S.splittable_resnet(cfg, skips_avgpool=False, skips_fc=False, num_classes=1000)
    _randomise_bn(model)
    x = torch.randn(2, 256, 56, 56).to(BF16)
    model.eval().to(dev).set_compute_dtype('bf16')
    with torch.no_grad():
        out = model.head(x.to(dev).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 1000) and bool(torch.isfinite(out.float()).all())
    return out


def layer3_input_gradient(S, dev):
    from sc2bench_amd.frozen import FrozenStack, FrozenStackFn
    from sc2bench_amd.resnet import resnet50
    torch.manual_seed(3)
    layer = resnet50().layer3
    _randomise_bn(layer)
    layer.eval()
    for p in layer.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 512, 28, 28).to(BF16)
    g = torch.randn(2, 1024, 14, 14).to(BF16)
    stack = FrozenStack('layer3', layer.to(dev))
    xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = FrozenStackFn.apply(xd, stack)
    out.backward(g.to(dev).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert xd.grad.shape == x.shape and bool(torch.isfinite(xd.grad.float()).all()) and float(xd.grad.float().abs().max()) > 0
    return xd.grad


def digests(S, dev):
    return {'head_logits': _sha(head_logits(S, dev)), 'layer3_input_gradient': _sha(layer3_input_gradient(S, dev))}


def test_head_bits(S, dev):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = digests(S, dev)
    print(got)
    assert got == want


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    import sc2bench_amd
    print(json.dumps(digests(sc2bench_amd, torch.device('cuda:0')), indent=1, sort_keys=True))
