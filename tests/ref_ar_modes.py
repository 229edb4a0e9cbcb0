"""TEST INFRASTRUCTURE ONLY: the operating point of the tests of mbt2018's codec modes (tests/test_ar_modes_cpu.py,
tests/test_gpu_ar_modes.py), fixed and seeded like ref_split_input.build, and the oracle's chain on it.

Oracle: tests/ref_input_hyperprior.JointAutoregressiveHierarchicalPriors(N = 32, M = 40): 10M/3 = 133 -> 136 and 8M/3 = 106 -> 112
exercise the zero padding of the packed widths, every channel count is a multiple of 4.  Every GDN's gamma 0.1 I + 0.02 rand, the
last layers of g_a / h_a / h_s scaled to std(y) = 4, std(z) = 3, std(params) = 2, entropy_parameters[4] scaled to std(gp) = 2 (gp of
the parallel path on round(y)) with +2 on the scale half's bias, update() called.  Images: torch.rand(4, 3, 64, 128): y is 4 x 8,
z is 1 x 2."""
import torch
from torch import nn

import ref_input_hyperprior as RH
import ref_split_input as ri

N_CH, M_CH = 32, 40
N_IMAGES = 4
PRECISE = {'f32': 'f64', 'bf16x3': 2, 'bf16x6': 3}       # encoder mode -> the arithmetic of ref_split_input.run_seq restating it


def images():
    return torch.rand(N_IMAGES, 3, 64, 128, generator=torch.Generator().manual_seed(1234))


def build(seed=0):
    """The oracle model at the operating point, updated, in eval mode."""
    torch.manual_seed(seed)
    model = RH.JointAutoregressiveHierarchicalPriors(N=N_CH, M=M_CH).eval()
    g = torch.Generator().manual_seed(seed + 1)
    x = images()
    eb, gc = model.entropy_bottleneck, model.gaussian_conditional
    with torch.no_grad():
        for seq in (model.g_a, model.g_s):
            for m in seq:
                if hasattr(m, 'gamma_reparam'):
                    C = m.beta.shape[0]
                    m.gamma.copy_(m.gamma_reparam.init(0.1 * torch.eye(C) + 0.02 * torch.rand(C, C, generator=g)))

        def scale_last(seq, run, std):
            last = [m for m in seq if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))][-1]
            s = std / run().std().item()
            last.weight.mul_(s)
            last.bias.mul_(s)
            return run()

        y = scale_last(model.g_a, lambda: model.g_a(x), 4.0)
        z = scale_last(model.h_a, lambda: model.h_a(y), 3.0)
        params = scale_last(model.h_s, lambda: model.h_s(eb.quantize(z, 'dequantize', ri.medians(eb, z))), 2.0)
        y_hat = gc.quantize(y, 'dequantize')
        scale_last(model.entropy_parameters, lambda: model.gaussian_params(params, y_hat), 2.0)
        model.entropy_parameters[4].bias[:M_CH] += 2.0
    model.update(force=True)
    return model


def chain(model, x):
    """The oracle's compress, stage by stage, in the model's own dtype (f32, or f64 after .double()):
    -> dict(y, z, z_sym, z_hat, params, strings, y_sym [B, H*W*M], idx, y_hat, x_hat [before the clamp])."""
    eb = model.entropy_bottleneck
    x = x.to(model.g_a[0].weight.dtype)
    with torch.no_grad():
        y = model.g_a(x)
        z = model.h_a(y)
        z_hat = eb.quantize(z, 'dequantize', ri.medians(eb, z))
        params = model.h_s(z_hat)
        strings, y_sym, idx, y_hat = model.compress_ar(y, params)
        x_hat = model.g_s(y_hat)
    return {'y': y, 'z': z, 'z_sym': eb.symbols(z).int(), 'z_hat': z_hat, 'params': params, 'strings': strings, 'y_sym': y_sym,
            'idx': idx, 'y_hat': y_hat.contiguous(), 'x_hat': x_hat}


def identical_images(a, b):
    """Per image: z symbols, indexes and y symbols of chain `a` equal chain `b`'s."""
    return [bool(torch.equal(a['z_sym'][i], b['z_sym'][i]) and torch.equal(a['idx'][i], b['idx'][i]) and
                 torch.equal(a['y_sym'][i], b['y_sym'][i])) for i in range(a['y_sym'].shape[0])]


_WORLD = {}


def world(seed=0):
    """(oracle, images, its f32 chain), built once per process: read-only."""
    if seed not in _WORLD:
        ref = build(seed)
        x = images()
        _WORLD[seed] = (ref, x, chain(ref, x))
    return _WORLD[seed]
