"""Restatement of the split-bf16 encoder modes ('bf16x3', 'bf16x6') in CPU torch ops: test infrastructure only.

Every f32 operand is written as a sum of `ns` bf16 numbers (hi = bf16(x), lo = bf16(x - hi), lo2 = bf16(x - hi - lo)); a convolution
is the sum of the part convolutions (i, j) with i + j <= ns - 1.  Each product of two bf16 numbers is exact in f32, so `acc`
(the dtype the part convolutions run and are summed in) only sets how the exact products are added up."""
import torch
import torch.nn.functional as F


def split(t, n):
    """f32 tensor -> n f32 tensors holding bf16 values."""
    parts, r = [], t.clone()
    for _ in range(n):
        p = r.to(torch.bfloat16).float()
        parts.append(p)
        r = r - p
    return parts


def split_conv(x, w, stride, pad, ns, acc=torch.float32):
    """part pairs with i + j <= ns - 1"""
    xs, ws = split(x, ns), split(w, ns)
    return sum(F.conv2d(xs[i].to(acc), ws[j].to(acc), None, stride, pad)
               for i in range(ns) for j in range(ns) if i + j <= ns - 1)


def gdn_params(gdn):
    """effective (gamma [C, C, 1, 1], beta [C]) of an oracle / device GDN1 module, f32 on the CPU"""
    C = gdn.beta.shape[0]
    with torch.no_grad():
        return (gdn.gamma_reparam(gdn.gamma).float().cpu().reshape(C, C, 1, 1), gdn.beta_reparam(gdn.beta).float().cpu())


def split_gdn(gdn, h, ns, acc=torch.float32):
    """GDN1 with the 1x1 convolution over |h| as a split convolution: norm = split_conv(|h|, gamma) + beta; h / norm (h * norm)."""
    gamma, beta = gdn_params(gdn)
    norm = split_conv(h.abs(), gamma, 1, 0, ns, acc).float() + beta.view(1, -1, 1, 1)
    return h * norm if gdn.inverse else h / norm


def split_encoder(oracle_bottleneck, x, ns, acc=torch.float32):
    """conv -> GDN1 -> conv -> GDN1 -> conv of the oracle bottleneck's encoder, every intermediate rounded to f32."""
    h = x.float()
    with torch.no_grad():
        for mod in oracle_bottleneck.encoder:
            if isinstance(mod, torch.nn.Conv2d):
                assert mod.bias is None and mod.stride[0] == mod.stride[1] and mod.padding[0] == mod.padding[1]
                h = split_conv(h, mod.weight.detach().float(), mod.stride[0], mod.padding[0], ns, acc).float()
            else:
                h = split_gdn(mod, h, ns, acc).float()
    return h
