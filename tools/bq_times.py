"""CR+BQ baseline (custom_resnet50: larger_resnet_bottleneck, 12 channels, split at 7, 8-bit quantizer, layer3 .. fc) at 256 images
of 224 x 224: ms per batch of the encoder (+ quantizer), of decoder + task head, and of the whole eval forward --

    hip    the package's eval path: bf16 kernels of libsc2amd.so (set_compute_dtype('bf16'))
    torch  the same weights as plain f32 torch modules and a torch-op quantizer (what the reference runs), same device

measured in this one process, the two alternating, R rounds (default 3), device events around K forwards each; then the per-kernel
rows of one hip forward from `hip.KernelTimer`.  Needs no data: random images, random weights, randomised norm statistics.

    python tools/bq_times.py [--rounds R] [--batch N]
"""
import argparse
import collections
import copy
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc2bench_amd as S  # noqa: E402
from sc2bench_amd import hip  # noqa: E402
from sc2bench_amd.transforms import Compose  # noqa: E402

Q = collections.namedtuple('Q', ['tensor', 'scale', 'zero_point'])


class TorchQuantizer(nn.Module):
    """the reference's quantize_tensor as torch ops on the input's device (one host read for the zero point, as upstream)"""

    def forward(self, x):
        low, high = x.min(), x.max()
        scale = (high - low) / 255.0
        zero_point = int((0.0 - low / scale).clamp(0.0, 255.0))
        return Q((zero_point + x / scale).clamp_(0.0, 255.0).round_().byte(), scale, zero_point)


class TorchDequantizer(nn.Module):
    def forward(self, q):
        return q.scale * (q.tensor.float() - q.zero_point)


def build(dev):
    torch.manual_seed(0)
    m = S.custom_resnet50(compressor=Compose([S.SimpleQuantizer(8)]), decompressor=Compose([S.SimpleDequantizer(8)]), num_classes=1000)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                n = mod.num_features
                mod.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(n, generator=g))
                mod.weight.copy_(torch.where(torch.rand(n, generator=g) < 0.3, -1.0, 1.0) * (0.5 + torch.rand(n, generator=g)))
                mod.bias.copy_(0.3 * torch.randn(n, generator=g))
    t = copy.deepcopy(m)
    t.bottleneck_layer.bottleneck_idx = None          # no known geometry: the plain torch modules
    t.bottleneck_layer.compressor, t.bottleneck_layer.decompressor = TorchQuantizer(), TorchDequantizer()
    t.use_hip_head = False
    m.eval().to(dev).set_compute_dtype('bf16')
    t.eval().to(dev)
    return m, t


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bq_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    m, t = build(dev)
    x = torch.rand(args.batch, 3, 224, 224, device=dev)
    stages = collections.OrderedDict()
    for name, model, iters in (('hip', m, 10), ('torch', t, 3)):
        bl = model.bottleneck_layer
        enc = [None]

        def encode(bl=bl, enc=enc):
            enc[0] = bl.encode(x)

        def decode_head(bl=bl, enc=enc, model=model):
            model.head(bl.decode(**enc[0]))

        def whole(model=model):
            model(x)
        stages[name] = (iters, collections.OrderedDict((('encode', encode), ('decode+head', decode_head), ('forward', whole))))
    rows = {(n, s): [] for n in stages for s in ('encode', 'decode+head', 'forward')}
    with torch.no_grad():
        for name, (iters, fns) in stages.items():      # warm-up: folded weights, code objects, the library's algorithm choices
            for fn in fns.values():
                fn()
                fn()
        for _ in range(args.rounds):
            for name, (iters, fns) in stages.items():
                for stage, fn in fns.items():
                    rows[(name, stage)].append(timed(fn, iters))
        out_h, out_t = m(x).float(), t(x).float()
    print('CR+BQ custom_resnet50 (12 channels, idx 7, 8 bits), batch {} x 3 x 224 x 224, device {}'.format(args.batch, torch.cuda.get_device_name(0)))
    print('ms per batch, {} alternating rounds (hip: 10 forwards per round, torch f32: 3)'.format(args.rounds))
    for stage in ('encode', 'decode+head', 'forward'):
        h, tt = rows[('hip', stage)], rows[('torch', stage)]
        print('{:<12} hip {}   torch {}   images/s hip {:.0f}  torch {:.0f}'.format(
            stage, ' '.join('{:8.3f}'.format(v) for v in h), ' '.join('{:8.3f}'.format(v) for v in tt),
            args.batch / min(h) * 1e3, args.batch / min(tt) * 1e3))
    s = out_t.abs().max().item()
    print('logits: max |hip - torch| {:.4f} at max |torch| {:.3f}; top-1 agreement {:.3f}'.format(
        (out_h - out_t).abs().max().item(), s, (out_h.argmax(1) == out_t.argmax(1)).float().mean().item()))
    with torch.no_grad(), hip.KernelTimer() as timer:
        for _ in range(5):
            m(x)
        torch.cuda.synchronize()
    total = 0.0
    print('per-kernel rows of the hip forward (mean of 5, ms):')
    for tag, (count, ms) in sorted(timer.summary().items(), key=lambda kv: -kv[1][1]):
        total += ms * count / 5
        print('  {:<28} {:8.4f}'.format(tag, ms))
    print('  {:<28} {:8.4f}'.format('sum of launches', total))


if __name__ == '__main__':
    main()
