"""TEST INFRASTRUCTURE ONLY: f32 CPU restatement of CompressAI 1.2.x's ScaleHyperprior, MeanScaleHyperprior and
JointAutoregressiveHierarchicalPriors (`compressai/models/google.py`, zoo names bmshj2018_hyperprior / mbt2018_mean /
mbt2018), including the per-pixel `_compress_ar` / `_decompress_ar` loops of the autoregressive model.

The architectures are [recalled], not read from a CompressAI install (none is importable here).  GDN, the convolution
helpers and the entropy bottleneck come from oracle.cpu_ref_input / oracle.cpu_ref, the Gaussian conditional from
oracle.cpu_ref, the rANS encoder from oracle.rans.  The per-pixel decoder needs a stream decoder that keeps its state between
pixels (upstream's RansDecoder.set_stream / decode_stream); `StreamDecoder` below states it.
"""
import struct

import torch
import torch.nn.functional as F
from torch import nn

from oracle import rans as oracle_rans
from oracle.cpu_ref import EntropyBottleneck, GaussianConditional, get_scale_table
from oracle.cpu_ref_input import GDN, _conv, _deconv

HYPERPRIOR_CFGS = {q: ((128, 192) if q <= 5 else (192, 320)) for q in range(1, 9)}
MEAN_SCALE_CFGS = {q: ((128, 192) if q <= 4 else (192, 320)) for q in range(1, 9)}
MBT2018_CFGS = {q: ((192, 192) if q <= 4 else (192, 320)) for q in range(1, 9)}

RANS64_L = 1 << 31


class StreamDecoder(object):
    """RansDecoder.set_stream(string) + decode_stream(indexes, cdfs, cdf_sizes, offsets) (64-bit state, 32-bit words,
    16-bit precision, 4-bit bypass escapes)."""

    def __init__(self, string):
        n = len(string) // 4
        self.words = list(struct.unpack('<{}I'.format(n), string[:4 * n]))
        self.pos = 2
        self.x = self._word(0) | (self._word(1) << 32)

    def _word(self, i):
        return self.words[i] if i < len(self.words) else 0

    def _renorm(self):
        if self.x < RANS64_L:
            self.x = (self.x << 32) | self._word(self.pos)
            self.pos += 1

    def _bits(self):
        v = self.x & 15
        self.x >>= 4
        self._renorm()
        return v

    def decode_stream(self, indexes, cdfs, cdf_sizes, offsets):
        out = []
        for idx in indexes:
            cdf, size = cdfs[idx], cdf_sizes[idx]
            max_value = size - 2
            cum = self.x & 0xFFFF
            s = 0
            while s + 1 < size and cdf[s + 1] <= cum:
                s += 1
            self.x = (cdf[s + 1] - cdf[s]) * (self.x >> 16) + cum - cdf[s]
            self._renorm()
            value = s
            if value == max_value:
                val = self._bits()
                n_bypass = val
                while val == 15:
                    val = self._bits()
                    n_bypass += val
                raw = 0
                for j in range(n_bypass):
                    raw |= self._bits() << (4 * j)
                value = raw >> 1
                value = -value - 1 if raw & 1 else value + max_value
            out.append(value + offsets[idx])
        return out


class MaskedConv2d(nn.Conv2d):
    def __init__(self, *args, mask_type='A', **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer('mask', torch.ones_like(self.weight.data))
        _, _, h, w = self.mask.size()
        self.mask[:, :, h // 2, w // 2 + (mask_type == 'B'):] = 0
        self.mask[:, :, h // 2 + 1:] = 0

    def forward(self, x):
        return F.conv2d(x, self.weight * self.mask, self.bias, self.stride, self.padding)


class _Base(nn.Module):
    def __init__(self, N, M):
        super().__init__()
        self.entropy_bottleneck = EntropyBottleneck(N)
        self.g_a = nn.Sequential(_conv(3, N), GDN(N), _conv(N, N), GDN(N), _conv(N, N), GDN(N), _conv(N, M))
        self.g_s = nn.Sequential(_deconv(M, N), GDN(N, inverse=True), _deconv(N, N), GDN(N, inverse=True),
                                 _deconv(N, N), GDN(N, inverse=True), _deconv(N, 3))
        self.gaussian_conditional = GaussianConditional(None)
        self.N, self.M = N, M

    def update(self, force=False):
        self.gaussian_conditional.update_scale_table(get_scale_table(), force=force)
        return self.entropy_bottleneck.update(force=force)

    def _tables(self):
        gc = self.gaussian_conditional
        return gc._quantized_cdf.tolist(), gc._cdf_length.reshape(-1).int().tolist(), gc._offset.reshape(-1).int().tolist()


class ScaleHyperprior(_Base):
    def __init__(self, N, M):
        super().__init__(N, M)
        self.h_a = nn.Sequential(_conv(M, N, 3, 1), nn.ReLU(inplace=True), _conv(N, N), nn.ReLU(inplace=True), _conv(N, N))
        self.h_s = nn.Sequential(_deconv(N, N), nn.ReLU(inplace=True), _deconv(N, N), nn.ReLU(inplace=True),
                                 _conv(N, M, 3, 1), nn.ReLU(inplace=True))

    def _hyper_in(self, y):
        return torch.abs(y)

    def _gaussian(self, params):
        return params, None

    def forward(self, x):
        y = self.g_a(x)
        z = self.h_a(self._hyper_in(y))
        z_hat, z_lik = self.entropy_bottleneck(z)
        scales, means = self._gaussian(self.h_s(z_hat))
        y_hat, y_lik = self.gaussian_conditional(y, scales, means=means)
        return {'x_hat': self.g_s(y_hat), 'likelihoods': {'y': y_lik, 'z': z_lik}}

    def compress(self, x):
        y = self.g_a(x)
        z = self.h_a(self._hyper_in(y))
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        scales, means = self._gaussian(self.h_s(z_hat))
        indexes = self.gaussian_conditional.build_indexes(scales)
        y_strings = self.gaussian_conditional.compress(y, indexes, means=means)
        return {'strings': [y_strings, z_strings], 'shape': z.size()[-2:]}

    def decompress(self, strings, shape):
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        scales, means = self._gaussian(self.h_s(z_hat))
        indexes = self.gaussian_conditional.build_indexes(scales)
        y_hat = self.gaussian_conditional.decompress(strings[0], indexes, means=means)
        return {'x_hat': self.g_s(y_hat).clamp_(0, 1)}


class MeanScaleHyperprior(ScaleHyperprior):
    def __init__(self, N, M):
        super().__init__(N, M)
        self.h_a = nn.Sequential(_conv(M, N, 3, 1), nn.LeakyReLU(inplace=True), _conv(N, N), nn.LeakyReLU(inplace=True),
                                 _conv(N, N))
        self.h_s = nn.Sequential(_deconv(N, M), nn.LeakyReLU(inplace=True), _deconv(M, M * 3 // 2), nn.LeakyReLU(inplace=True),
                                 _conv(M * 3 // 2, M * 2, 3, 1))

    def _hyper_in(self, y):
        return y

    def _gaussian(self, params):
        return params.chunk(2, 1)


class JointAutoregressiveHierarchicalPriors(MeanScaleHyperprior):
    def __init__(self, N=192, M=192):
        super().__init__(N, M)
        self.entropy_parameters = nn.Sequential(
            nn.Conv2d(M * 12 // 3, M * 10 // 3, 1), nn.LeakyReLU(inplace=True),
            nn.Conv2d(M * 10 // 3, M * 8 // 3, 1), nn.LeakyReLU(inplace=True),
            nn.Conv2d(M * 8 // 3, M * 6 // 3, 1))
        self.context_prediction = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)

    def gaussian_params(self, params, y_hat):
        """The parallel context path: entropy_parameters(cat(params, context_prediction(y_hat)))."""
        return self.entropy_parameters(torch.cat((params, self.context_prediction(y_hat)), dim=1))

    def forward(self, x):
        y = self.g_a(x)
        z = self.h_a(y)
        z_hat, z_lik = self.entropy_bottleneck(z)
        params = self.h_s(z_hat)
        y_hat = self.gaussian_conditional.quantize(y, 'dequantize')
        scales, means = self.gaussian_params(params, y_hat).chunk(2, 1)
        _, y_lik = self.gaussian_conditional(y, scales, means=means)
        return {'x_hat': self.g_s(y_hat), 'likelihoods': {'y': y_lik, 'z': z_lik}}

    def _step(self, y_hat, params, h, w, kernel_size=5):
        y_crop = y_hat[:, :, h:h + kernel_size, w:w + kernel_size]
        cp = self.context_prediction
        ctx_p = F.conv2d(y_crop, cp.weight * cp.mask, bias=cp.bias)
        p = params[:, :, h:h + 1, w:w + 1]
        gp = self.entropy_parameters(torch.cat((p, ctx_p), dim=1)).squeeze(3).squeeze(2)
        scales_hat, means_hat = gp.chunk(2, 1)
        return y_crop, scales_hat, means_hat

    def compress_ar(self, y, params, padding=2):
        """-> (list of one bytes per image, symbols [B, H*W*M] and indexes pixel-major, the final y_hat NCHW)."""
        cdf, cdf_len, offsets = self._tables()
        y_hat = F.pad(y, (padding,) * 4)
        H, W = y.shape[-2:]
        syms, idxs = [[] for _ in range(y.shape[0])], [[] for _ in range(y.shape[0])]
        for h in range(H):
            for w in range(W):
                y_crop, scales_hat, means_hat = self._step(y_hat, params, h, w)
                indexes = self.gaussian_conditional.build_indexes(scales_hat)
                y_q = self.gaussian_conditional.quantize(y_crop[:, :, padding, padding], 'symbols', means_hat)
                y_hat[:, :, h + padding, w + padding] = y_q + means_hat
                for b in range(y.shape[0]):
                    syms[b].extend(y_q[b].int().tolist())
                    idxs[b].extend(indexes[b].tolist())
        strings = [oracle_rans.encode_with_indexes(syms[b], idxs[b], cdf, cdf_len, offsets) for b in range(y.shape[0])]
        return strings, torch.tensor(syms, dtype=torch.int32), torch.tensor(idxs, dtype=torch.int32), \
            y_hat[:, :, padding:-padding, padding:-padding]

    def decompress_ar(self, strings, params, padding=2):
        cdf, cdf_len, offsets = self._tables()
        B, _, H, W = params.shape
        y_hat = torch.zeros((B, self.M, H + 2 * padding, W + 2 * padding))
        decs = [StreamDecoder(s) for s in strings]
        for h in range(H):
            for w in range(W):
                _, scales_hat, means_hat = self._step(y_hat, params, h, w)
                indexes = self.gaussian_conditional.build_indexes(scales_hat)
                for b in range(B):
                    rv = torch.tensor(decs[b].decode_stream(indexes[b].tolist(), cdf, cdf_len, offsets), dtype=torch.float32)
                    y_hat[b, :, h + padding, w + padding] = rv + means_hat[b]
        return y_hat[:, :, padding:-padding, padding:-padding]

    def compress(self, x):
        y = self.g_a(x)
        z = self.h_a(y)
        z_strings = self.entropy_bottleneck.compress(z)
        z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
        y_strings = self.compress_ar(y, self.h_s(z_hat))[0]
        return {'strings': [y_strings, z_strings], 'shape': z.size()[-2:]}

    def decompress(self, strings, shape):
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        y_hat = self.decompress_ar(strings[0], self.h_s(z_hat))
        return {'x_hat': self.g_s(y_hat).clamp_(0, 1)}


ZOO = {'bmshj2018_hyperprior': (ScaleHyperprior, HYPERPRIOR_CFGS), 'mbt2018_mean': (MeanScaleHyperprior, MEAN_SCALE_CFGS),
       'mbt2018': (JointAutoregressiveHierarchicalPriors, MBT2018_CFGS)}


def build(name, quality):
    cls, cfgs = ZOO[name]
    return cls(*cfgs[quality])
