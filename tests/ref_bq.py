"""The CR+BQ baseline written down once more, on torch CPU ops in f32: the contract the package's kernels and modules are
tested against (tests/test_bq_cpu.py, test_gpu_bq_kernels.py, test_gpu_bq.py).

* `quantize` / `dequantize`: torchdistill's `tensor_util.quantize_tensor(x, 8)` / `dequantize_tensor`, step by step on 0-dim f32
  tensors, so every step is one IEEE f32 operation:
      scale = (max - min) / 255;  izp = 0 - min / scale;  zp = int(clamp(izp, 0, 255))  [int(nan) raises ValueError];
      q = (zp + x / scale).clamp(0, 255).round().byte()        [round: half to even]
      x' = scale * (q.float() - zp)
* `Bottleneck`: the 20-module sequence of the reference's `larger_resnet_bottleneck`, split at `idx`, with the same
  state-dict keys (`encoder.N.*`, `decoder.N.*`), plain torch modules, no compressor logic beyond calling it.
Nothing here imports the package under test.
"""
import collections

import torch
from torch import nn

Quantized = collections.namedtuple('Quantized', ['tensor', 'scale', 'zero_point'])


def quantize(x):
    """x: f32 CPU tensor -> Quantized(u8 tensor, 0-dim f32 scale, int zero point)"""
    assert x.dtype == torch.float32 and not x.is_cuda
    low, high = x.min(), x.max()
    scale = (high - low) / 255.0
    izp = 0.0 - low / scale
    if izp < 0.0:
        zp = 0.0
    elif izp > 255.0:
        zp = 255.0
    else:
        zp = izp
    zp = int(zp)            # ValueError on NaN, as the reference
    q = zp + x / scale
    q = q.clamp(0.0, 255.0).round().to(torch.uint8)
    return Quantized(q, scale, zp)


def dequantize(q):
    return q.scale * (q.tensor.float() - q.zero_point)


def quantize_per_sample(x):
    return [quantize(x[i]) for i in range(x.shape[0])]


def modules(channels):
    def conv(cin, cout, k, s, p):
        return nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p, bias=False)
    seq = [conv(3, 64, 7, 2, 3), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(3, 2, 1), nn.BatchNorm2d(64), nn.ReLU(),
           conv(64, channels, 2, 2, 1), nn.BatchNorm2d(channels), nn.ReLU()]
    for cin, pad in ((channels, 1), (512, 1), (512, 0)):
        seq += [conv(cin, 512, 2, 1, pad), nn.BatchNorm2d(512), nn.ReLU()]
    seq += [conv(512, 512, 2, 1, 0), nn.AvgPool2d(2, 1)]
    assert len(seq) == 20
    return seq


class Bottleneck(nn.Module):
    def __init__(self, channels=12, idx=7, quantized=True):
        super().__init__()
        seq = modules(channels)
        self.encoder = nn.Sequential(*seq[:idx])
        self.decoder = nn.Sequential(*seq[idx:])
        self.quantized = quantized

    def encode(self, x):
        z = self.encoder(x)
        return quantize(z) if self.quantized else z

    def decode(self, z):
        return self.decoder(dequantize(z) if self.quantized else z)

    def forward(self, x):
        if self.training:
            return self.decoder(self.encoder(x))
        return self.decode(self.encode(x))


def randomise_norms(module, seed=0):
    """running statistics away from (0, 1) and affine weights of both signs in every BatchNorm2d of `module`"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.5 + torch.rand(n, generator=g))
                sign = torch.where(torch.rand(n, generator=g) < 0.3, -1.0, 1.0)
                m.weight.copy_(sign * (0.5 + torch.rand(n, generator=g)))
                m.bias.copy_(0.3 * torch.randn(n, generator=g))
    return module


# ---- edge sets of the quantizer (each with the scale bits / zero point the restatement must give: asserted before any launch)
def ties_set(n):
    """min -64 and max 191 planted (scale exactly 1.0, zero point 64), every other value k + 0.5: codes round half to even"""
    assert n >= 2
    x = (torch.arange(n, dtype=torch.float32) % 200) - 60.0 + 0.5     # -59.5 .. 139.5
    x[0], x[-1] = -64.0, 191.0
    return x


def edge_sets(n, seed=0):
    """{name: (f32 tensor of n elements, expected zero point or None, expected scale or None)}"""
    g = torch.Generator().manual_seed(seed + n)
    r = torch.randn(n, generator=g)
    first = 3.0 * r.clone()
    first[0], first[-1] = -20.0, 17.0
    last = 3.0 * r.clone()
    last[0], last[-1] = 17.0, -20.0
    return {
        'randn': (3.0 * r, None, None),
        'negative': (-(r.abs()) - 0.5, 255, None),
        'positive': (r.abs() + 0.5, 0, None),
        'ties': (ties_set(n), 64, 1.0),
        'extremes_first_last': (first, None, None),
        'extremes_last_first': (last, None, None),
        'const_pos': (torch.full((n,), 1.5), 0, 0.0),
        'const_neg': (torch.full((n,), -1.5), 255, 0.0),
    }
