"""Restatement of the neural input codecs' transforms (FactorizedPrior, ScaleHyperprior, MeanScaleHyperprior: g_a, h_a, h_s, g_s
with biased convolutions / transposed convolutions and the squared-form GDN) in CPU torch ops, in the arithmetic of each codec
mode: test infrastructure only.  Extends tests/ref_split_encoder.py and tests/ref_split_hyper.py (imported, not edited).

  'f32'   the oracle's own torch ops (oracle.cpu_ref_input / tests/ref_input_hyperprior.py), its torch.rsqrt included
  'f64'   every convolution summed in f64 and rounded once to f32: the target of set_encoder_precision('f32')
  2 / 3   every operand as a sum of 2 / 3 bf16 parts, the part convolutions (i, j) with i + j <= ns - 1 ('bf16x3' / 'bf16x6')

The restatements ('f64', 2, 3) add the bias to the ROUNDED f32 sum and take the squared GDN as the device does: norm = sum + beta,
r = sqrt(norm), then h * r (inverse) or h * (1.0 / r).  Every intermediate is rounded to f32.

`build(name)` fixes the operating point of the tests (seeded): N = 128, M = 192 (the quality-1 configurations), every GDN's gamma
0.1 I + 0.02 rand (so the 1x1 is a real reduction), the last layers of g_a / h_a / h_s scaled to std(y) = 4, std(z) = 3,
std(params) = 2 on `images()` = torch.rand(4, 3, 128, 192) (not square on purpose: y is 8 x 12, z is 2 x 3)."""
import torch
import torch.nn.functional as F
from torch import nn

import ref_split_encoder as rs
import ref_split_hyper as rh

NAMES = ('FactorizedPrior', 'ScaleHyperprior', 'MeanScaleHyperprior')
N_CH, M_CH = 128, 192
N_IMAGES = 4


def _gdn2(m, h, conv1x1):
    gamma, beta = rs.gdn_params(m)
    norm = conv1x1(h * h, gamma) + beta.view(1, -1, 1, 1)
    r = torch.sqrt(norm)
    return h * r if m.inverse else h * (1.0 / r)


def _ops(mode, acc):
    """-> (conv, conv_transpose, gdn) of a restated mode; each returns the f32 value (no bias)."""
    if mode == 'f64':
        return (lambda h, w, s, p: F.conv2d(h.double(), w.double(), None, s, p).float(),
                lambda h, w, s, p, op: F.conv_transpose2d(h.double(), w.double(), None, s, p, op).float(),
                lambda m, h: _gdn2(m, h, lambda t, g: F.conv2d(t.double(), g.double()).float()))
    ns = int(mode)
    assert ns in (2, 3)
    return (lambda h, w, s, p: rs.split_conv(h, w, s, p, ns, acc).float(),
            lambda h, w, s, p, op: rh.split_conv_transpose(h, w, s, p, ns, acc, op).float(),
            lambda m, h: _gdn2(m, h, lambda t, g: rs.split_conv(t, g, 1, 0, ns, acc).float()))


def run_seq(mods, h, mode, acc=torch.float32):
    """An oracle nn.Sequential of (biased) Conv2d / ConvTranspose2d / GDN / ReLU / LeakyReLU in the arithmetic of `mode`."""
    h = h.float()
    with torch.no_grad():
        if mode == 'f32':
            for m in mods:
                h = F.leaky_relu(h, m.negative_slope) if isinstance(m, nn.LeakyReLU) else (F.relu(h) if isinstance(m, nn.ReLU) else m(h))
            return h
        conv, conv_t, gdn = _ops(mode, acc)
        for m in mods:
            if isinstance(m, (nn.ConvTranspose2d, nn.Conv2d)):
                assert m.stride[0] == m.stride[1] and m.padding[0] == m.padding[1]
                w = m.weight.detach().float()
                if isinstance(m, nn.ConvTranspose2d):
                    h = conv_t(h, w, m.stride[0], m.padding[0], m.output_padding[0])
                else:
                    h = conv(h, w, m.stride[0], m.padding[0])
                if m.bias is not None:
                    h = h + m.bias.detach().float().view(1, -1, 1, 1)
            elif isinstance(m, nn.LeakyReLU):
                h = F.leaky_relu(h, m.negative_slope)
            elif isinstance(m, nn.ReLU):
                h = F.relu(h)
            elif hasattr(m, 'gamma_reparam'):
                h = gdn(m, h)
            else:
                raise RuntimeError('restatement: unexpected module {}'.format(type(m).__name__))
    return h


def has_hyper(model):
    return hasattr(model, 'h_a')


def is_mean_scale(model):
    return type(model).__name__ == 'MeanScaleHyperprior'


def medians(eb, t):
    m = eb._extend_ndims(eb._get_medians().detach(), t.ndim - 2)
    return m.expand(t.size(0), *([-1] * (t.ndim - 1)))


def stages(model, x, mode, inputs=None, acc=torch.float32, y=None):
    """The transforms of an oracle input codec (updated) in the arithmetic of `mode`.  inputs = None: the chain end to end (each
    stage fed this mode's own values).  inputs = a dict from an earlier call (the oracle's, mode 'f32'): each stage fed THAT call's
    input (stage-wise: g_a on x, h_a on its y, h_s on its z_hat, g_s on its y_hat).  y: this mode's g_a(x) from an earlier call.
    -> dict(y, y_sym, y_hat, x_hat [before the clamp]; hyperprior models also z, z_sym, z_hat, params, scales, means, idx)."""
    eb = model.entropy_bottleneck
    out = {}
    with torch.no_grad():
        y = run_seq(model.g_a, x, mode, acc) if y is None else y
        if has_hyper(model):
            gc = model.gaussian_conditional
            y_in = y if inputs is None else inputs['y']
            z = run_seq(model.h_a, y_in if is_mean_scale(model) else y_in.abs(), mode, acc)
            z_hat = eb.quantize(z, 'dequantize', medians(eb, z))
            params = run_seq(model.h_s, z_hat if inputs is None else inputs['z_hat'], mode, acc)
            scales, means = params.chunk(2, 1) if is_mean_scale(model) else (params, None)
            mu = means if inputs is None else inputs['means']      # (stage-wise: this mode's y around the oracle's means)
            out.update(z=z, z_sym=eb.symbols(z).int(), z_hat=z_hat, params=params, scales=scales, means=means,
                       idx=gc.build_indexes(scales).int())
            y_sym = gc.quantize(y, 'symbols', mu)
            y_hat = gc.quantize(y, 'dequantize', mu)
        else:
            y_sym = eb.symbols(y)
            y_hat = eb.quantize(y, 'dequantize', medians(eb, y))
        x_hat = run_seq(model.g_s, y_hat if inputs is None else inputs['y_hat'], mode, acc)
        out.update(y=y, y_sym=y_sym.int(), y_hat=y_hat, x_hat=x_hat)
    return out


def int_tensors(s):
    """The integer tensors that decide the bytes: (z symbols, indexes, y symbols), or (y symbols,) of the factorized model."""
    return (s['z_sym'], s['idx'], s['y_sym']) if 'idx' in s else (s['y_sym'],)


identical_images = rh.identical_images


def images():
    return torch.rand(N_IMAGES, 3, 128, 192, generator=torch.Generator().manual_seed(1234))


def build(name, seed=0):
    """The oracle model `name` (one of NAMES) at the tests' operating point, updated, in eval mode."""
    from oracle import cpu_ref_input
    import ref_input_hyperprior
    assert name in NAMES
    torch.manual_seed(seed)
    cls = cpu_ref_input.FactorizedPrior if name == 'FactorizedPrior' else getattr(ref_input_hyperprior, name)
    model = cls(N_CH, M_CH).eval()
    g = torch.Generator().manual_seed(seed + 1)
    x = images()
    with torch.no_grad():
        for seq in (model.g_a, model.g_s):
            for m in seq:
                if hasattr(m, 'gamma_reparam'):
                    C = m.beta.shape[0]
                    m.gamma.copy_(m.gamma_reparam.init(0.1 * torch.eye(C) + 0.02 * torch.rand(C, C, generator=g)))

        def scale_last(seq, t_in, std):
            last = [m for m in seq if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))][-1]
            s = std / seq(t_in).std().item()
            last.weight.mul_(s)
            if last.bias is not None:
                last.bias.mul_(s)
            return seq(t_in)

        y = scale_last(model.g_a, x, 4.0)
        if has_hyper(model):
            eb = model.entropy_bottleneck
            z = scale_last(model.h_a, y if is_mean_scale(model) else y.abs(), 3.0)
            scale_last(model.h_s, eb.quantize(z, 'dequantize', medians(eb, z)), 2.0)
    model.update(force=True)
    return model


# --------------------------------------------------------------------------------------------- #
# the squared GDN on integers (zero tolerance: tests/test_gpu_precise_gdn2.py; its CPU conditions: tests/test_input_modes_cpu.py)
# --------------------------------------------------------------------------------------------- #
GDN2_CHANNELS = (12, 100, 128, 192)       # one partial tile; the tail tile of a second chunk; 96 + 32; two full chunks
GDN2_PIXELS = ((1, 1, 1), (2, 5, 7))      # one pixel; 70 pixels (not a tile multiple)


def gdn2_int_case(C, pixels):
    """x in {-3..3} [N,C,H,W], gamma in {0, 1, 2} [C,C], beta integers in 1..4 [C] (all f32, bf16-exact), and the exact integer
    norm = gamma x^2 + beta as f32 [N,C,H,W] (<= 192 * 2 * 9 + 4: exact in f32 in every summation order and in every mode)."""
    N, H, W = pixels
    g = torch.Generator().manual_seed(C * 1000 + N * 100 + H * 10 + W)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
    gamma = torch.randint(0, 3, (C, C), generator=g).float()
    beta = torch.randint(1, 5, (C,), generator=g).float()
    norm64 = F.conv2d((x * x).double(), gamma.double().view(C, C, 1, 1)) + beta.double().view(1, -1, 1, 1)
    norm = norm64.float()
    assert torch.equal(norm.double(), norm64) and float(norm.max()) < (1 << 24) and float(norm.min()) >= 1
    return x, gamma, beta, norm


def gdn2_int_expected(x, norm, inverse):
    """The device's operation order in correctly rounded f32 operations on the CPU: r = sqrt(norm); x * r (inverse) or x * (1 / r).
    sqrt and the division run in f64 on the f32 operands and are rounded ONCE to f32, which is the correctly rounded f32 result
    (53 >= 2 * 24 + 2 bits; tests/test_input_modes_cpu.py proves it on these values with exact products).  torch's own f32 sqrt
    is not used: its AVX-512 vector path is not correctly rounded (sqrt(267), sqrt(999): the same test counts them)."""
    r = torch.sqrt(norm.double()).float()
    return x * r if inverse else x * (1.0 / r.double()).float()
