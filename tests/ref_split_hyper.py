"""Restatement of the hyperprior codec chain (g_a -> h_a -> z symbols -> h_s -> indexes, y symbols) in CPU torch ops, in the
arithmetic of each codec mode: test infrastructure only.  Extends tests/ref_split_encoder.py (imported, not edited).

  'f32'   the oracle's own arithmetic: torch's CPU f32 convolutions (what the reference computes)
  'f64'   every convolution summed in f64 and rounded once to f32: the target of set_encoder_precision('f32'), whose kernel is a
          k-ordered f32 fma chain (f32-grade, another summation order than torch's)
  2 / 3   every operand as a sum of 2 / 3 bf16 parts, the part pairs with i + j <= ns - 1 ('bf16x3' / 'bf16x6'), each part
          convolution in `acc` (f32: the device's accumulator type; f64: the exact sum of the same products)

Activations run on the f32 value (F.relu / F.leaky_relu: v > 0 ? v : v * 0.01f), every intermediate is rounded to f32."""
import torch
import torch.nn.functional as F
from torch import nn

import ref_split_encoder as rs


def split_conv_transpose(x, w, stride, pad, ns, acc=torch.float32, output_padding=0):
    """conv_transpose2d as the sum of the part transposed convolutions (i, j) with i + j <= ns - 1; w: [Cin, Cout, KH, KW]."""
    xs, ws = rs.split(x, ns), rs.split(w, ns)
    return sum(F.conv_transpose2d(xs[i].to(acc), ws[j].to(acc), None, stride, pad, output_padding)
               for i in range(ns) for j in range(ns) if i + j <= ns - 1)


def _ops(mode, acc):
    """-> (conv, conv_transpose, gdn) of a mode; each returns f32."""
    if mode == 'f32':
        return (lambda h, w, s, p: F.conv2d(h, w, None, s, p),
                lambda h, w, s, p, op: F.conv_transpose2d(h, w, None, s, p, op),
                lambda m, h: m(h))
    if mode == 'f64':
        def gdn(m, h):
            gamma, beta = rs.gdn_params(m)
            norm = F.conv2d(h.abs().double(), gamma.double()).float() + beta.view(1, -1, 1, 1)
            return h * norm if m.inverse else h / norm
        return (lambda h, w, s, p: F.conv2d(h.double(), w.double(), None, s, p).float(),
                lambda h, w, s, p, op: F.conv_transpose2d(h.double(), w.double(), None, s, p, op).float(),
                gdn)
    ns = int(mode)
    assert ns in (2, 3)
    return (lambda h, w, s, p: rs.split_conv(h, w, s, p, ns, acc).float(),
            lambda h, w, s, p, op: split_conv_transpose(h, w, s, p, ns, acc, op).float(),
            lambda m, h: rs.split_gdn(m, h, ns, acc).float())


def run_seq(mods, h, mode, acc=torch.float32):
    """An oracle nn.Sequential of Conv2d / ConvTranspose2d / GDN1 / ReLU / LeakyReLU in the arithmetic of `mode`."""
    conv, conv_t, gdn = _ops(mode, acc)
    h = h.float()
    with torch.no_grad():
        for m in mods:
            if isinstance(m, nn.ConvTranspose2d):
                assert m.bias is None and m.stride[0] == m.stride[1] and m.padding[0] == m.padding[1]
                h = conv_t(h, m.weight.detach().float(), m.stride[0], m.padding[0], m.output_padding[0])
            elif isinstance(m, nn.Conv2d):
                assert m.bias is None and m.stride[0] == m.stride[1] and m.padding[0] == m.padding[1]
                h = conv(h, m.weight.detach().float(), m.stride[0], m.padding[0])
            elif isinstance(m, nn.LeakyReLU):
                h = F.leaky_relu(h, m.negative_slope)
            elif isinstance(m, nn.ReLU):
                h = F.relu(h)
            elif hasattr(m, 'gamma_reparam'):
                h = gdn(m, h)
            else:
                raise RuntimeError('restatement: unexpected module {}'.format(type(m).__name__))
    return h


def is_mean_scale(bl):
    return type(bl).__name__.startswith('MSHP')


def stages(bl, x, mode, inputs=None, acc=torch.float32, y=None):
    """The three transforms of an oracle hyperprior bottleneck `bl` (updated) in the arithmetic of `mode`.
    inputs = None: the chain end to end (each stage fed this mode's own values).  inputs = a dict from an earlier call (the
    oracle's, mode 'f32'): each stage fed THAT call's input (stage-wise comparison).
    y: this mode's g_a(x) from an earlier call (g_a is the expensive stage), else it is computed.
    -> dict(y, z, z_hat, params, scales, means, z_sym, idx, y_sym): floats f32, integers int32."""
    eb, gc = bl.entropy_bottleneck, bl.gaussian_conditional
    with torch.no_grad():
        y = run_seq(bl.g_a, x, mode, acc) if y is None else y
        y_in = y if inputs is None else inputs['y']
        z = run_seq(bl.h_a, y_in if is_mean_scale(bl) else y_in.abs(), mode, acc)
        z_sym = eb.symbols(z)
        z_hat = eb.quantize(z, 'dequantize', bl._get_means(z))
        params = run_seq(bl.h_s, z_hat if inputs is None else inputs['z_hat'], mode, acc)
        scales, means = params.chunk(2, 1) if is_mean_scale(bl) else (params, None)
        idx = gc.build_indexes(scales)
        # (stage-wise: the y symbols of THIS mode's g_a around the oracle's means, as the device test quantises)
        mu = means if inputs is None else inputs['means']
        y_sym = gc.quantize(y, 'symbols', mu)
    return dict(y=y, z=z, z_hat=z_hat, params=params, scales=scales, means=means, z_sym=z_sym.int(), idx=idx.int(),
                y_sym=y_sym.int())


def chain(bl, x, mode, acc=torch.float32):
    """-> (z symbols, indexes, y symbols) of the whole chain in the arithmetic of `mode`."""
    s = stages(bl, x, mode, acc=acc)
    return s['z_sym'], s['idx'], s['y_sym']


def identical_images(a, b):
    """Images whose three integer tensors (z symbols, indexes, y symbols) all agree: -> list of bool."""
    n = a[0].shape[0]
    return [all(bool(torch.equal(u[i], v[i])) for u, v in zip(a, b)) for i in range(n)]


def shape_like_bench(bl):
    """The operating point benchlib.workloads gives the mshp224 model, on an oracle OR device bottleneck in place; the SHP twin's
    one-headed h_s gets abs() * 5 on the whole tail weight."""
    with torch.no_grad():
        eb = bl.entropy_bottleneck
        q = torch.zeros(eb.quantiles.shape[0], 1, 3)
        for c in range(q.shape[0]):
            q[c, 0, 0], q[c, 0, 1], q[c, 0, 2] = -(3 + c % 5), 0.25 * (c % 3), 4 + c % 7
        eb.quantiles.copy_(q)
        bl.g_a[4].weight.mul_(10.0)
        bl.h_a[2].weight.mul_(4.0)
        w = bl.h_s[4].weight
        if is_mean_scale(bl):
            w[:w.shape[0] // 2].abs_().mul_(5.0)
        else:
            w.abs_().mul_(5.0)
    return bl
