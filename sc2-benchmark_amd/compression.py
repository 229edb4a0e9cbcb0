"""Learned image-compression models for the neural INPUT compression baselines of the reference
(configs/ilsvrc2012/input_compression/factorized_prior-resnet50.yaml:60-65: `bmshj2018_factorized`, quality 8;
scale_hyperprior-*.yaml, mean_scale_hyperprior-*.yaml and joint_autoregressive_hierarchical_prior-*.yaml:
`bmshj2018_hyperprior`, `mbt2018_mean`, `mbt2018`), built through sc2bench/models/registry.py:58-105 from CompressAI's
zoo and driven by `NeuralInputCompressionClassifier`, sc2bench/models/wrapper.py:80-135.

`FactorizedPrior` keeps CompressAI's architecture, parameter / buffer names and API (`forward`, `compress`,
`decompress`, `update`, `aux_loss`, `load_state_dict`): g_a = 4 x Conv(k5, s2, p2, bias) with 3 GDN in between,
g_s = 4 x ConvTranspose(k5, s2, p2, output_padding 1, bias) with 3 inverse GDN, an `EntropyBottleneck(M)` on the latent.
Every tensor-sized computation runs in the HIP library: the convolutions / transposed convolutions on the implicit-GEMM
MFMA kernel (bias in the epilogue), GDN as a 1x1 GEMM on x^2 with rsqrt / sqrt fused in the epilogue, the entropy
bottleneck and the range coder as in the supervised-compression bottleneck.

`set_encoder_precision('f32' | 'bf16x3' | 'bf16x6')` (or the constructor's `encoder_precision=`) moves every transform of
`FactorizedPrior`, `ScaleHyperprior` and `MeanScaleHyperprior` to the precise kernels (csrc/conv_f32.hip / conv_split.hip) on
f32 activations: see `_PrecisionSwitch`.  `JointAutoregressiveHierarchicalPriors` (`mbt2018`) takes them once its serial context scan
reads f32 weights (`set_scan_precision('f32')`, a switch of its own): see the class.
"""
import functools

import torch
from torch import nn

from . import hip
from .entropy import (CompressionModel, EntropyBottleneck, GaussianConditional, GDN, HipConv2d, HipConvTranspose2d,
                      _raise_on_status, _require_device, get_scale_table, run_hip_transform_precise, update_registered_buffers)

COMPRESSION_MODEL_CLASS_DICT = dict()
COMPRESSION_MODEL_FUNC_DICT = dict()


def register_compression_model_class(cls):
    COMPRESSION_MODEL_CLASS_DICT[cls.__name__] = cls
    return cls


def register_compression_model_func(func):
    COMPRESSION_MODEL_FUNC_DICT[func.__name__] = func
    return func


def conv(in_channels, out_channels, kernel_size=5, stride=2):
    return HipConv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2)


def deconv(in_channels, out_channels, kernel_size=5, stride=2):
    return HipConvTranspose2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                              output_padding=stride - 1, padding=kernel_size // 2)


def _run_transform(seq, x_nhwc, last_out_format):
    h = x_nhwc
    n = len(seq)
    for i, m in enumerate(seq):
        fmt = last_out_format if i == n - 1 else hip.OUT_BF16_NHWC
        h = m.forward_nhwc(h, out_format=fmt)
    return h


_SPLIT_PARTS = {'bf16x3': 2, 'bf16x6': 3}   # encoder precision -> bf16 parts per operand (csrc/conv_split.hip)


class _PrecisionSwitch(object):
    """`set_encoder_precision` of the input codecs: the four names (and the ValueError) of FPBasedResNetBottleneck's switch."""
    encoder_precision = 'bf16'

    def set_encoder_precision(self, precision):
        """'bf16' (default): every transform with bf16 operands and bf16 activations on the implicit-GEMM kernel, as ever.
        'f32': f32 operands on the f32 matrix cores (csrc/conv_f32.hip); 'bf16x3' / 'bf16x6': f32 activations and weights as
        sums of two / three bf16 parts on the bf16 matrix cores (csrc/conv_split.hip).
        As in the hyperprior bottlenecks the mode is a property of the CODEC: g_a decides the y symbols, h_a the z symbols, h_s
        the CDF-row index of every y symbol (and the means), which the decoder rebuilds from the decoded z.  In the three precise
        modes g_a, h_a, h_s AND g_s (the reconstruction is what a user of an image codec measures, and upstream's is f32) run on
        the precise kernels in every path: forward, compress, decompress and FactorizedPrior's stage_front / stage_coder /
        stage_back.  The squared-form GDN is norm = gamma x^2 + beta, sqrt, one division, one multiply, all correctly rounded
        (csrc/conv_precise.h).  The hyper-latent, y_hat and the means travel as f32: neither symbols + medians nor symbols +
        means is bf16-exact.
        A stream made in one mode is only guaranteed to decode in THAT mode: another mode's h_s may put a scale on the other side
        of a scale-table boundary, and one wrong index desynchronises the range decoder for the rest of the image.  Set the same
        mode on both ends."""
        if precision not in ('bf16', 'f32') + tuple(_SPLIT_PARTS):
            raise ValueError("encoder precision must be 'bf16', 'f32', 'bf16x3' or 'bf16x6', got {!r}".format(precision))
        self.encoder_precision = precision
        return self

    def _precise_ns(self):
        """None in 'bf16' mode, else the bf16 parts per operand of the precise kernels (0: f32 operands)."""
        if self.encoder_precision == 'bf16':
            return None
        return _SPLIT_PARTS.get(self.encoder_precision, 0)

    def _nhwc(self, t):
        """f32 NCHW -> the NHWC form this mode's transforms take: bf16, or f32 in the precise modes."""
        if self._precise_ns() is not None:
            return hip.nchw_f32_to_nhwc_f32(t.float().contiguous())
        return hip.nchw_f32_to_nhwc_bf16(t.float().contiguous(), t.shape[1])


@register_compression_model_class
class FactorizedPrior(_PrecisionSwitch, CompressionModel):
    """Factorized-prior model of Balle et al. 2018 as packaged by CompressAI (`compressai.models.FactorizedPrior`).

    :param N: channels of the transforms
    :param M: channels of the latent
    :param encoder_precision: 'bf16' (default), 'f32', 'bf16x3' or 'bf16x6': `set_encoder_precision`
    """

    def __init__(self, N, M, encoder_precision='bf16', **kwargs):
        super().__init__(entropy_bottleneck_channels=M)
        self.set_encoder_precision(encoder_precision)
        self.g_a = nn.Sequential(
            conv(3, N), GDN(N),
            conv(N, N), GDN(N),
            conv(N, N), GDN(N),
            conv(N, M),
        )
        self.g_s = nn.Sequential(
            deconv(M, N), GDN(N, inverse=True),
            deconv(N, N), GDN(N, inverse=True),
            deconv(N, N), GDN(N, inverse=True),
            deconv(N, 3),
        )
        self.N = N
        self.M = M
        for prefix, seq in (('g_a', self.g_a), ('g_s', self.g_s)):
            for i, mod in enumerate(seq):
                mod._tag = '{}.{}'.format(prefix, i)

    @property
    def downsampling_factor(self):
        return 2 ** 4

    # ---- transforms on the device ---------------------------------------------------------------- #
    def analysis(self, x, slice_bytes=0x7FF00000 - 1):
        """g_a(x): f32 NCHW image batch -> f32 NCHW latent.  slice_bytes (precise modes): the largest f32 tensor of a launch."""
        _require_device(x, 'FactorizedPrior')
        ns = self._precise_ns()
        if ns is not None:      # the image as it is: ns = 0 reads the three planes in place
            return run_hip_transform_precise(self.g_a, x.float().contiguous(), ns, x_is_nchw_rgb=True, slice_bytes=slice_bytes)
        x_nhwc = hip.nchw_f32_to_nhwc_bf16(x.float().contiguous(), 8)
        return _run_transform(self.g_a, x_nhwc, hip.OUT_F32_NCHW)

    def synthesis_nhwc(self, y_hat_nhwc, slice_bytes=0x7FF00000 - 1):
        """g_s on an NHWC latent (bf16; f32 in the precise modes) -> f32 NCHW reconstruction."""
        ns = self._precise_ns()
        if ns is not None:
            if y_hat_nhwc.dtype != torch.float32:
                raise hip.Sc2Error('synthesis: mode {!r} takes the f32 latent'.format(self.encoder_precision))
            return run_hip_transform_precise(self.g_s, y_hat_nhwc, ns, slice_bytes=slice_bytes)
        out = _run_transform(self.g_s, y_hat_nhwc, hip.OUT_F32_NHWC)
        return out.permute(0, 3, 1, 2).contiguous()

    def synthesis(self, y_hat, **kwargs):
        _require_device(y_hat, 'FactorizedPrior')
        return self.synthesis_nhwc(self._nhwc(y_hat), **kwargs)

    # ---- CompressAI API ---------------------------------------------------------------------------- #
    def forward(self, x):
        y = self.analysis(x)
        y_hat, y_likelihoods = self.entropy_bottleneck(y)
        x_hat = self.synthesis(y_hat)
        return {'x_hat': x_hat, 'likelihoods': {'y': y_likelihoods}}

    def compress(self, x):
        y = self.analysis(x)
        y_strings = self.entropy_bottleneck.compress(y)
        return {'strings': [y_strings], 'shape': y.size()[-2:]}

    def decompress(self, strings, shape):
        assert isinstance(strings, list) and len(strings) == 1
        if self._precise_ns() is not None:     # symbols + medians is not bf16-exact: y_hat stays f32
            y_hat = self.entropy_bottleneck.decompress_to_device(strings[0], tuple(shape), want_f32=True, want_nhwc=False)[0]
            return {'x_hat': self.synthesis(y_hat).clamp_(0, 1)}
        _, y_hat_nhwc = self.entropy_bottleneck.decompress_to_device(strings[0], tuple(shape), want_f32=False, want_nhwc=True)
        x_hat = self.synthesis_nhwc(y_hat_nhwc).clamp_(0, 1)
        return {'x_hat': x_hat}

    # ---- compress -> decompress in stages (pipeline.StagePipeline through NeuralInputCompressionClassifier)
    stage_front_takes_out = False

    def stage_front(self, x, out=None):
        y = self.analysis(x)
        return self.entropy_bottleneck.symbols_device(y), tuple(y.shape[-2:])

    def stage_coder(self, sym, hw_shape, dequantized=False):
        eb = self.entropy_bottleneck
        hw = hw_shape[0] * hw_shape[1]
        buf, off, nb, st = eb.encode_symbols_device(sym, hw)
        if dequantized and self._precise_ns() is None:      # (the fused pass writes a bf16 y_hat: the precise modes hand on symbols)
            y_hat = eb.decode_dequantize_device(buf, off, nb, sym.shape[1], hw_shape)
            if y_hat is not None:
                return y_hat, nb, st
        return eb.decode_symbols_device(buf, off, nb, sym.shape[1], hw), nb, st

    def stage_back(self, decoded, hw_shape):
        if self._precise_ns() is not None:
            if decoded.dtype != torch.int32:
                raise hip.Sc2Error('stage_back: mode {!r} takes the decoded symbols, not a {} latent'.format(self.encoder_precision,
                                                                                                             decoded.dtype))
            y_hat = self.entropy_bottleneck.dequantize_device(decoded, hw_shape, want_f32=True, want_nhwc=False)[0]
            return self.synthesis(y_hat).clamp_(0, 1)
        y_hat = decoded if decoded.dtype == torch.bfloat16 else self.entropy_bottleneck.dequantize_device(decoded, hw_shape)[1]
        return self.synthesis_nhwc(y_hat).clamp_(0, 1)

    @classmethod
    def from_state_dict(cls, state_dict):
        N = state_dict['g_a.0.weight'].size(0)
        M = state_dict['g_a.6.weight'].size(0)
        net = cls(N, M)
        net.load_state_dict(state_dict)
        return net


# compressai.zoo.image: quality -> (N, M) of bmshj2018-factorized
FACTORIZED_CFGS = {1: (128, 192), 2: (128, 192), 3: (128, 192), 4: (128, 192), 5: (128, 192),
                   6: (192, 320), 7: (192, 320), 8: (192, 320)}


@register_compression_model_func
def bmshj2018_factorized(quality, metric='mse', pretrained=False, progress=True, **kwargs):
    """compressai.zoo.bmshj2018_factorized.  Pretrained weights are downloaded upstream; offline they are read from
    $SC2_PRETRAINED_DIR/bmshj2018-factorized-{metric}-{quality}.pth (a CompressAI state dict, old `_matrix{i}` key names
    accepted) -- if that file is absent the model keeps its random initialisation and says so."""
    import logging
    import os
    import warnings
    if metric not in ('mse', 'ms-ssim'):
        raise ValueError('Invalid metric "{}"'.format(metric))
    if quality < 1 or quality > 8:
        raise ValueError('Invalid quality "{}", should be between (1, 8)'.format(quality))
    model = FactorizedPrior(*FACTORIZED_CFGS[quality], **kwargs)
    if pretrained:
        root = os.environ.get('SC2_PRETRAINED_DIR')
        path = os.path.join(root, 'bmshj2018-factorized-{}-{}.pth'.format(metric, quality)) if root else None
        if path and os.path.isfile(path):
            from .ckpt import _torch_load
            model.load_state_dict(_torch_load(path))
        else:
            msg = ('bmshj2018_factorized(quality={}, pretrained=True): no local weights ({}); the model is RANDOMLY '
                   'INITIALISED'.format(quality, path or 'SC2_PRETRAINED_DIR unset'))
            if os.environ.get('SC2_STRICT_WEIGHTS') == '1':
                raise FileNotFoundError(msg)
            warnings.warn(msg)
            logging.getLogger(__name__).warning(msg)
    return model


# --------------------------------------------------------------------------------------------- #
# hyperprior models (compressai.models.google: ScaleHyperprior, MeanScaleHyperprior,
# JointAutoregressiveHierarchicalPriors) -- the architecture is [recalled] from CompressAI 1.2.x, not read from an install
# --------------------------------------------------------------------------------------------- #
def _pad8(c):
    return (c + 7) // 8 * 8


def _run_biased(seq, x_nhwc, a_op=hip.AOP_NONE, last_out_format=hip.OUT_F32_NCHW):
    """An nn.Sequential of biased HipConv2d / HipConvTranspose2d with ReLU / LeakyReLU(0.01) in between (the h_a / h_s
    transforms of the hyperprior models) on bf16 NHWC activations: bias and activation ride in the conv's epilogue.  `a_op`
    applies to the first conv's input (|y| of the scale hyperprior)."""
    mods = list(seq)
    h = x_nhwc
    i = 0
    while i < len(mods):
        m = mods[i]
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        epi = hip.EPI_BIAS
        if isinstance(nxt, nn.ReLU):
            epi = hip.EPI_BIAS_RELU
        elif isinstance(nxt, nn.LeakyReLU):
            if abs(nxt.negative_slope - 0.01) > 1e-12:
                raise hip.Sc2Error('LeakyReLU({}): only a slope of 0.01 is fused'.format(nxt.negative_slope))
            epi = hip.EPI_BIAS_LEAKY_RELU
        last = i + (2 if epi != hip.EPI_BIAS else 1) >= len(mods)
        fmt = last_out_format if last else hip.OUT_BF16_NHWC
        if isinstance(m, HipConvTranspose2d):
            if i == 0 and a_op != hip.AOP_NONE:
                raise hip.Sc2Error('_run_biased: an input operand on a transposed convolution')
            if h.shape[-1] != m.in_channels:
                raise hip.Sc2Error('_run_biased: {} channels into {}'.format(h.shape[-1], m))
            kfmt = hip.OUT_F32_NHWC if fmt == hip.OUT_F32_NCHW else fmt
            # an output width that is no multiple of 8 (3M/2 = 60 at M = 40) stays zero-padded for the convolution behind it
            h = m.forward_nhwc(h, hip.EPI_NONE if epi == hip.EPI_BIAS else epi, None, out_format=kfmt, keep_pad=not last)
            if fmt == hip.OUT_F32_NCHW:
                h = h.permute(0, 3, 1, 2).contiguous()
        elif isinstance(m, HipConv2d):
            assert m.bias is not None
            if h.shape[-1] == m.in_channels:
                w, order = m.packed_weight(), m.k_order()
            elif h.shape[-1] == _pad8(m.in_channels):       # zero channels from the padded layer before: zero weight columns
                w, order = m.padded_weight(h.shape[-1]), hip.K_TAP_MAJOR
            else:
                raise hip.Sc2Error('_run_biased: {} channels into {}'.format(h.shape[-1], m))
            h = hip.conv2d_fwd(h, w, m.out_channels, m.kernel_size[0], m.kernel_size[1], m.stride,
                               m.padding, a_op=a_op if i == 0 else hip.AOP_NONE, epilogue=epi, ep_beta=m.bias_f32(),
                               out_format=fmt, tag=getattr(m, '_tag', None), k_order=order)
        else:
            raise hip.Sc2Error('_run_biased: unsupported module {}'.format(type(m).__name__))
        i += 1 if epi == hip.EPI_BIAS else 2
    return h


def _tag(prefix, seq):
    for i, mod in enumerate(seq):
        mod._tag = '{}.{}'.format(prefix, i)


class _HyperpriorBase(_PrecisionSwitch, CompressionModel):
    """g_a / g_s as in FactorizedPrior, an EntropyBottleneck(N) on z and a GaussianConditional on y.  `encoder_precision`:
    'bf16' (default), 'f32', 'bf16x3' or 'bf16x6' (`set_encoder_precision`)."""

    def __init__(self, N, M, encoder_precision='bf16', **kwargs):
        super().__init__(entropy_bottleneck_channels=N)
        self.set_encoder_precision(encoder_precision)
        self.g_a = nn.Sequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
        self.g_s = nn.Sequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                                 deconv(N, N), GDN(N, inverse=True), deconv(N, 3))
        self.gaussian_conditional = GaussianConditional(None)
        self.N = int(N)
        self.M = int(M)

    def _tag_all(self):
        for name in ('g_a', 'g_s', 'h_a', 'h_s'):
            _tag(name, getattr(self, name))

    @property
    def downsampling_factor(self):
        return 2 ** (4 + 2)

    analysis = FactorizedPrior.analysis
    synthesis_nhwc = FactorizedPrior.synthesis_nhwc
    synthesis = FactorizedPrior.synthesis

    def hyper_analysis(self, y):
        """h_a(|y|) (scale hyperprior) or h_a(y): f32 NCHW y -> f32 NCHW z."""
        a_op = hip.AOP_ABS if self._hyper_abs else hip.AOP_NONE
        ns = self._precise_ns()
        if ns is not None:
            return run_hip_transform_precise(self.h_a, self._nhwc(y), ns, a_op=a_op)
        return _run_biased(self.h_a, self._nhwc(y), a_op=a_op)

    def hyper_synthesis(self, z_hat_nhwc, out_format=hip.OUT_F32_NCHW):
        """h_s on an NHWC hyper-latent (bf16; f32 in the precise modes) -> the Gaussian parameters."""
        ns = self._precise_ns()
        if ns is not None:
            if z_hat_nhwc.dtype != torch.float32:
                raise hip.Sc2Error('hyper_synthesis: mode {!r} takes the f32 hyper-latent'.format(self.encoder_precision))
            return run_hip_transform_precise(self.h_s, z_hat_nhwc, ns, out_format=out_format)
        return _run_biased(self.h_s, z_hat_nhwc, last_out_format=out_format)

    def _z_hat_nhwc(self, z_strings, shape):
        if self._precise_ns() is not None:      # symbols + medians is not bf16-exact: the hyper-latent stays f32
            return self._nhwc(self.entropy_bottleneck.decompress_to_device(z_strings, tuple(shape), want_f32=True, want_nhwc=False)[0])
        return self.entropy_bottleneck.decompress_to_device(z_strings, tuple(shape), want_f32=False, want_nhwc=True)[1]

    def update(self, scale_table=None, force=False, update_quantiles=False):
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        updated |= self.entropy_bottleneck.update(force=force, update_quantiles=update_quantiles)
        return updated

    def load_state_dict(self, state_dict, strict=True):
        update_registered_buffers(self.gaussian_conditional, 'gaussian_conditional',
                                  ['_quantized_cdf', '_offset', '_cdf_length', 'scale_table'], state_dict)
        return super().load_state_dict(state_dict, strict=strict)

    @classmethod
    def from_state_dict(cls, state_dict):
        N = state_dict['g_a.0.weight'].size(0)
        M = state_dict['g_a.6.weight'].size(0)
        net = cls(N, M)
        net.load_state_dict(state_dict)
        return net

    # ---- the y stream of the two non-autoregressive models
    def _gaussian(self, params):
        return params, None

    def forward(self, x):
        y = self.analysis(x)
        z = self.hyper_analysis(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales_hat, means_hat = self._gaussian(self.hyper_synthesis(self._nhwc(z_hat)))
        y_hat, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        x_hat = self.synthesis(y_hat)
        return {'x_hat': x_hat, 'likelihoods': {'y': y_likelihoods, 'z': z_likelihoods}}

    def compress(self, x):
        y = self.analysis(x)
        z = self.hyper_analysis(y)
        z_strings = self.entropy_bottleneck.compress(z)
        scales_hat, means_hat = self._gaussian(self.hyper_synthesis(self._z_hat_nhwc(z_strings, z.shape[-2:])))
        indexes = self.gaussian_conditional.build_indexes(scales_hat)
        y_strings = self.gaussian_conditional.compress(y, indexes, means=means_hat)
        return {'strings': [y_strings, z_strings], 'shape': z.size()[-2:]}

    def decompress(self, strings, shape):
        assert isinstance(strings, list) and len(strings) == 2
        scales_hat, means_hat = self._gaussian(self.hyper_synthesis(self._z_hat_nhwc(strings[1], shape)))
        indexes = self.gaussian_conditional.build_indexes(scales_hat)
        if self._precise_ns() is not None:     # symbols + means is not bf16-exact: y_hat stays f32
            y_hat = self.gaussian_conditional.decompress_to_device(strings[0], indexes, means_hat, want_f32=True,
                                                                   want_nhwc=False)[0]
            return {'x_hat': self.synthesis(y_hat).clamp_(0, 1)}
        y_hat_nhwc = self.gaussian_conditional.decompress_to_device(strings[0], indexes, means_hat, want_f32=False,
                                                                    want_nhwc=True)[1]
        return {'x_hat': self.synthesis_nhwc(y_hat_nhwc).clamp_(0, 1)}


@register_compression_model_class
class ScaleHyperprior(_HyperpriorBase):
    """Scale hyperprior of Balle et al. 2018 (`compressai.models.ScaleHyperprior`) [recalled]: h_a = conv(M, N, k3, s1) ReLU
    conv(N, N) ReLU conv(N, N) on |y|; h_s = deconv(N, N) ReLU deconv(N, N) ReLU conv(N, M, k3, s1) ReLU gives the scales.

    :param N: channels of the transforms
    :param M: channels of the latent
    """
    _hyper_abs = True

    def __init__(self, N, M, **kwargs):
        super().__init__(N, M, **kwargs)
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.ReLU(inplace=True), conv(N, N), nn.ReLU(inplace=True),
                                 conv(N, N))
        self.h_s = nn.Sequential(deconv(N, N), nn.ReLU(inplace=True), deconv(N, N), nn.ReLU(inplace=True),
                                 conv(N, M, stride=1, kernel_size=3), nn.ReLU(inplace=True))
        self._tag_all()


@register_compression_model_class
class MeanScaleHyperprior(_HyperpriorBase):
    """Mean-scale hyperprior of Minnen et al. 2018 (`compressai.models.MeanScaleHyperprior`) [recalled]: h_a with LeakyReLU
    on y; h_s = deconv(N, M) LReLU deconv(M, 3M/2) LReLU conv(3M/2, 2M, k3, s1), chunked into scales and means."""
    _hyper_abs = False

    def __init__(self, N, M, **kwargs):
        super().__init__(N, M, **kwargs)
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.LeakyReLU(inplace=True), conv(N, N),
                                 nn.LeakyReLU(inplace=True), conv(N, N))
        self.h_s = nn.Sequential(deconv(N, M), nn.LeakyReLU(inplace=True), deconv(M, M * 3 // 2), nn.LeakyReLU(inplace=True),
                                 conv(M * 3 // 2, M * 2, stride=1, kernel_size=3))
        self._tag_all()

    def _gaussian(self, params):
        scales_hat, means_hat = params.chunk(2, 1)
        return scales_hat, means_hat


class MaskedConv2d(HipConv2d):
    """compressai.layers.MaskedConv2d [recalled]: a Conv2d whose taps at and after the centre (mask type 'A'; 'B' keeps the
    centre) in raster order are zero.  `mask` is a registered buffer.  The device kernels read the masked weights, packed
    once per parameter version; the parameter itself is not rewritten."""

    def __init__(self, *args, mask_type='A', **kwargs):
        super().__init__(*args, **kwargs)
        if mask_type not in ('A', 'B'):
            raise ValueError('Invalid "mask_type" value "{}"'.format(mask_type))
        self.register_buffer('mask', torch.ones_like(self.weight.data))
        _, _, h, w = self.mask.size()
        self.mask[:, :, h // 2, w // 2 + (mask_type == 'B'):] = 0
        self.mask[:, :, h // 2 + 1:] = 0

    def masked_weight(self):
        return self.weight.detach() * self.mask

    def packed_weight(self, k_order=None):
        order = self.k_order() if k_order is None else k_order
        key = (self.weight._version, self.mask._version, self.weight.device, self.weight.data_ptr(), order)
        if self.__dict__.get('_masked_key') != key:
            self._masked_packed = hip.pack_conv_weight(self.masked_weight(), order)
            self._masked_key = key
        return self._masked_packed


@register_compression_model_class
class JointAutoregressiveHierarchicalPriors(MeanScaleHyperprior):
    """Joint autoregressive and hierarchical priors of Minnen et al. 2018 (`compressai.models.
    JointAutoregressiveHierarchicalPriors`, zoo name `mbt2018`) [recalled]: the mean-scale model's transforms plus a 5x5
    type-A masked context model (M -> 2M) and `entropy_parameters` = 1x1 convs 12M/3 -> 10M/3 -> 8M/3 -> 6M/3 with LeakyReLU.

    `forward` is the parallel form (context convolution over the whole dequantised map).  `compress` / `decompress` are the
    serial raster scan of upstream's `_compress_ar` / `_decompress_ar` on the device (csrc/ar_context.hip): one workgroup per
    image, the y stream of an image = ONE rANS stream of its symbols in pixel-major, channel-minor order with per-symbol
    Gaussian indexes.  The hyper-params half of the first entropy_parameters layer runs for all pixels before the scan, in
    both directions.  Channel counts that are not multiples of 8 (10M/3, 8M/3 at M = 320) are zero-padded in the packed
    weights and activations.

    Two precision switches, neither a parameter or buffer (state dicts are what they were):
    `set_scan_precision('bf16' | 'f32')` (kwarg `scan_precision`): the weight form of the serial scan.  'bf16' (default) reads the
    four matrices rounded to bf16, 'f32' reads them unrounded (sc2_ar_scan_f32: the same step code, twice the weight bytes per
    step).  The scan's precision is a codec property of its own: an f32 scan with bf16 transforms is a self-consistent codec.
    `set_encoder_precision` (kwarg `encoder_precision`): as on the other input codecs, but a precise mode ('f32' / 'bf16x3' /
    'bf16x6') is refused with Sc2Error while the scan is 'bf16' -- a codec precise in g_a / h_a / h_s alone would promise bytes it
    cannot keep -- and `set_scan_precision('bf16')` is refused while a precise mode is set.  In the precise modes g_a, h_a, h_s, g_s,
    the hyper-params half of entropy_parameters' first layer (p1) and `forward`'s context convolution and entropy_parameters run
    on the precise kernels with f32 NHWC activations; the scan is the f32 one in all three (it is VALU code: there is no matrix
    product to split).  A stream decodes only under the two settings that made it."""
    scan_precision = 'bf16'

    def set_scan_precision(self, precision):
        """'bf16' (default) or 'f32': the weight form the serial scan of compress / decompress reads.  -> self."""
        if precision not in ('bf16', 'f32'):
            raise ValueError("scan precision must be 'bf16' or 'f32', got {!r}".format(precision))
        if precision == 'bf16' and self.encoder_precision != 'bf16':
            raise hip.Sc2Error('JointAutoregressiveHierarchicalPriors: encoder precision {!r} needs the f32 context scan; set the '
                               "encoder precision to 'bf16' first".format(self.encoder_precision))
        self.scan_precision = precision
        return self

    def set_encoder_precision(self, precision):
        previous = self.encoder_precision
        super().set_encoder_precision(precision)     # (an unknown name: ValueError)
        if precision != 'bf16' and self.scan_precision != 'f32':
            self.encoder_precision = previous
            raise hip.Sc2Error('JointAutoregressiveHierarchicalPriors: encoder precision {!r} is not supported while the context scan '
                               "(csrc/ar_context.hip) has bf16 operands; set_scan_precision('f32') lifts this".format(precision))
        return self

    def __init__(self, N=192, M=192, scan_precision='bf16', **kwargs):
        if scan_precision not in ('bf16', 'f32'):
            raise ValueError("scan precision must be 'bf16' or 'f32', got {!r}".format(scan_precision))
        self.__dict__['scan_precision'] = scan_precision     # before the base class sets encoder_precision, whatever the kwarg order
        super().__init__(N, M, **kwargs)
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.LeakyReLU(inplace=True), conv(N, N),
                                 nn.LeakyReLU(inplace=True), conv(N, N))
        self.h_s = nn.Sequential(deconv(N, M), nn.LeakyReLU(inplace=True), deconv(M, M * 3 // 2), nn.LeakyReLU(inplace=True),
                                 conv(M * 3 // 2, M * 2, stride=1, kernel_size=3))
        self.entropy_parameters = nn.Sequential(
            HipConv2d(M * 12 // 3, M * 10 // 3, 1), nn.LeakyReLU(inplace=True),
            HipConv2d(M * 10 // 3, M * 8 // 3, 1), nn.LeakyReLU(inplace=True),
            HipConv2d(M * 8 // 3, M * 6 // 3, 1))
        self.context_prediction = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)
        self._tag_all()
        _tag('entropy_parameters', self.entropy_parameters)
        self.context_prediction._tag = 'context_prediction'

    @property
    def downsampling_factor(self):
        return 2 ** (4 + 2)

    # ---- packed weights (once per parameter version)
    def _padded_f32(self):
        """The f32 matrices every pack is cut from: entropy_parameters' 1x1 weights zero-padded to C1p / C2p (w1p [C1p, 4M], w2p
        [C2p, C1p], w3p [2M, C2p], b1 [C1p], b2 [C2p]) and the masked context weights k-major (wc [12M, 2M], k = tap * M + channel)."""
        ep = self.entropy_parameters
        cp = self.context_prediction
        M = self.M
        C1, C2 = ep[0].out_channels, ep[2].out_channels
        C1p, C2p = _pad8(C1), _pad8(C2)
        dev = cp.weight.device
        with torch.no_grad():
            w1 = ep[0].weight.detach().float()[:, :, 0, 0]          # [C1, 4M]
            w2 = ep[2].weight.detach().float()[:, :, 0, 0]          # [C2, C1]
            w3 = ep[4].weight.detach().float()[:, :, 0, 0]          # [2M, C2]
            b1 = torch.zeros(C1p, device=dev)
            b1[:C1] = ep[0].bias.detach().float()
            b2 = torch.zeros(C2p, device=dev)
            b2[:C2] = ep[2].bias.detach().float()
            w1p = torch.zeros(C1p, 4 * M, device=dev)
            w1p[:C1] = w1
            w2p = torch.zeros(C2p, C1p, device=dev)
            w2p[:C2, :C1] = w2
            w3p = torch.zeros(2 * M, C2p, device=dev)
            w3p[:, :C2] = w3
            mw = cp.masked_weight().float()                          # [2M, M, 5, 5]
            taps = [(ky, kx) for ky in range(2) for kx in range(5)] + [(2, 0), (2, 1)]
            wc = torch.cat([mw[:, :, ky, kx].t() for ky, kx in taps], 0)   # [12M, 2M], k = tap * M + channel
        return {'C1p': C1p, 'C2p': C2p, 'w1p': w1p, 'w2p': w2p, 'w3p': w3p, 'b1': b1, 'b2': b2, 'wc': wc, 'mw': mw}

    def _packed(self, scan_f32=False):
        """The packed weights of the current parameter versions.  scan_f32: also 'scan_f32', the scan's matrices masked, k-major and
        UNROUNDED (built when first asked for, dropped with the rest when a parameter changes)."""
        ep = self.entropy_parameters
        cp = self.context_prediction
        params = [cp.weight, cp.bias, cp.mask] + [p for i in (0, 2, 4) for p in (ep[i].weight, ep[i].bias)]
        key = tuple((p._version, p.data_ptr(), p.device) for p in params)
        if self.__dict__.get('_packed_key') != key:
            M = self.M
            f = self._padded_f32()
            C1p, C2p, w1p, w2p, w3p, b1, b2, wc = (f[k] for k in ('C1p', 'C2p', 'w1p', 'w2p', 'w3p', 'b1', 'b2', 'wc'))
            with torch.no_grad():
                pk = {
                    'C1p': C1p, 'C2p': C2p,
                    # the parallel path: 1x1 convs on the packed-weight kernels (zero rows / columns for the padding)
                    'ep1': hip.pack_conv_weight(w1p.reshape(C1p, 4 * M, 1, 1)), 'eb1': b1.contiguous(),
                    'ep2': hip.pack_conv_weight(w2p.reshape(C2p, C1p, 1, 1)), 'eb2': b2.contiguous(),
                    'ep3': hip.pack_conv_weight(w3p.reshape(2 * M, C2p, 1, 1)), 'eb3': ep[4].bias.detach().float().contiguous(),
                    # the hyper-params half of layer 1, for all pixels before the scan
                    'ep1a': hip.pack_conv_weight(w1p[:, :2 * M].contiguous().reshape(C1p, 2 * M, 1, 1)),
                    # the scan: k-major bf16
                    'scan': {'wc': wc.to(torch.bfloat16).contiguous(), 'bc': cp.bias.detach().float().contiguous(),
                             'w1': w1p[:, 2 * M:].t().to(torch.bfloat16).contiguous(),
                             'w2': w2p.t().to(torch.bfloat16).contiguous(), 'b2': b2.contiguous(),
                             'w3': w3p.t().to(torch.bfloat16).contiguous(), 'b3': ep[4].bias.detach().float().contiguous()},
                }
            self._packed_cache = pk
            self._packed_key = key
        pk = self._packed_cache
        if scan_f32 and 'scan_f32' not in pk:
            f = self._padded_f32()
            bf = pk['scan']
            pk['scan_f32'] = {'wc': f['wc'].contiguous(), 'bc': bf['bc'], 'w1': f['w1p'][:, 2 * self.M:].t().contiguous(),
                              'w2': f['w2p'].t().contiguous(), 'b2': bf['b2'], 'w3': f['w3p'].t().contiguous(), 'b3': bf['b3']}
        return pk

    def _scan_weights(self):
        """The scan's weight dict in the form `scan_precision` names."""
        if self.scan_precision == 'f32':
            return self._packed(scan_f32=True)['scan_f32']
        return self._packed()['scan']

    def _precise_pack(self, name):
        """Fragment-major weights of the precise kernels in the current mode for one of 'ctx' (masked 5x5), 'ep1', 'ep2', 'ep3'
        (padded 1x1) and 'ep1a' (the hyper-params half of layer 1); built when first needed, kept with the pack."""
        ns = self._precise_ns()
        if ns is None:
            raise hip.Sc2Error('JointAutoregressiveHierarchicalPriors: no precise weights in mode {!r}'.format(self.encoder_precision))
        if self.M % 4:
            raise hip.Sc2Error('JointAutoregressiveHierarchicalPriors: mode {!r} needs M to be a multiple of 4, got {}'.format(
                self.encoder_precision, self.M))
        pk = self._packed()
        if (name, ns) not in pk:
            f = self._padded_f32()
            M = self.M
            w = {'ctx': lambda: f['mw'], 'ep1': lambda: f['w1p'].reshape(f['C1p'], 4 * M, 1, 1),
                 'ep2': lambda: f['w2p'].reshape(f['C2p'], f['C1p'], 1, 1), 'ep3': lambda: f['w3p'].reshape(2 * M, f['C2p'], 1, 1),
                 'ep1a': lambda: f['w1p'][:, :2 * M].contiguous().reshape(f['C1p'], 2 * M, 1, 1)}[name]()
            with torch.no_grad():
                pk[(name, ns)] = hip.pack_conv_split(w, ns) if ns else hip.pack_conv_f32(w)
        return pk[(name, ns)]

    def _precise_conv(self, h, name, cout, k, pad, epilogue, bias, out_format, tag):
        """One launch of the precise kernels of the current mode on an f32 NHWC map."""
        ns = self._precise_ns()
        conv = functools.partial(hip.conv2d_split_fwd, ns=ns) if ns else hip.conv2d_f32_fwd
        sfx = '.bf16x{}'.format(3 * (ns - 1)) if ns else '.f32'
        return conv(h, self._precise_pack(name), cout, k, k, 1, pad, epilogue=epilogue, ep_beta=bias, out_format=out_format,
                    tag=tag + sfx)

    def entropy_parameters_nhwc(self, params_nhwc, ctx_nhwc):
        """entropy_parameters(cat(params, ctx)) on bf16 NHWC maps (f32 NHWC in the precise modes) -> f32 NCHW gaussian params
        [B, 2M, H, W]."""
        pk = self._packed()
        h = torch.cat([params_nhwc, ctx_nhwc], dim=3).contiguous()
        if self._precise_ns() is not None:       # f32 NHWC maps, LeakyReLU in the epilogue, the padded widths kept
            if h.dtype != torch.float32:
                raise hip.Sc2Error('entropy_parameters: mode {!r} takes f32 maps'.format(self.encoder_precision))
            h = self._precise_conv(h, 'ep1', pk['C1p'], 1, 0, hip.EPI_BIAS_LEAKY_RELU, pk['eb1'], hip.OUT_F32_NHWC, 'entropy_parameters.0')
            h = self._precise_conv(h, 'ep2', pk['C2p'], 1, 0, hip.EPI_BIAS_LEAKY_RELU, pk['eb2'], hip.OUT_F32_NHWC, 'entropy_parameters.2')
            return self._precise_conv(h, 'ep3', 2 * self.M, 1, 0, hip.EPI_BIAS, pk['eb3'], hip.OUT_F32_NCHW, 'entropy_parameters.4')
        h = hip.conv2d_fwd(h, pk['ep1'], pk['C1p'], 1, 1, 1, 0, epilogue=hip.EPI_BIAS_LEAKY_RELU, ep_beta=pk['eb1'],
                           tag='entropy_parameters.0')
        h = hip.conv2d_fwd(h, pk['ep2'], pk['C2p'], 1, 1, 1, 0, epilogue=hip.EPI_BIAS_LEAKY_RELU, ep_beta=pk['eb2'],
                           tag='entropy_parameters.2')
        return hip.conv2d_fwd(h, pk['ep3'], 2 * self.M, 1, 1, 1, 0, epilogue=hip.EPI_BIAS, ep_beta=pk['eb3'],
                              out_format=hip.OUT_F32_NCHW, tag='entropy_parameters.4')

    def context_nhwc(self, y_hat):
        """context_prediction(y_hat) over the whole map: f32 NCHW y_hat -> bf16 NHWC [B, H, W, 2M] (f32 NHWC in the precise modes)."""
        cp = self.context_prediction
        if self._precise_ns() is not None:
            return self._precise_conv(self._nhwc(y_hat), 'ctx', 2 * self.M, 5, 2, hip.EPI_BIAS, cp.bias_f32(), hip.OUT_F32_NHWC,
                                      'context_prediction')
        x = hip.nchw_f32_to_nhwc_bf16(y_hat.float().contiguous(), self.M)
        return hip.conv2d_fwd(x, cp.packed_weight(), 2 * self.M, 5, 5, 1, 2, epilogue=hip.EPI_BIAS, ep_beta=cp.bias_f32(),
                              tag='context_prediction', k_order=cp.k_order())

    def forward(self, x):
        y = self.analysis(x)
        z = self.hyper_analysis(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        if self._precise_ns() is not None:
            params = self.hyper_synthesis(self._nhwc(z_hat), out_format=hip.OUT_F32_NHWC)
        else:
            params = self.hyper_synthesis(hip.nchw_f32_to_nhwc_bf16(z_hat.contiguous(), self.N), out_format=hip.OUT_BF16_NHWC)
        y_hat = self.gaussian_conditional.quantize(y, 'noise' if self.training else 'dequantize')
        gaussian_params = self.entropy_parameters_nhwc(params, self.context_nhwc(y_hat))
        scales_hat, means_hat = gaussian_params.chunk(2, 1)
        _, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        x_hat = self.synthesis(y_hat)
        return {'x_hat': x_hat, 'likelihoods': {'y': y_likelihoods, 'z': z_likelihoods}}

    # ---- the serial scan
    def hyper_params_term(self, params_nhwc):
        """p1 = W1[:, :2M] . params + b1, the hyper-params half of entropy_parameters' first layer for every pixel, zero-padded to
        C1p: bf16 NHWC params (f32 NHWC in the precise modes: one precise 1x1 launch on the f32 params) -> f32 [B, H, W, C1p]."""
        pk = self._packed()
        if self._precise_ns() is not None:
            if params_nhwc.dtype != torch.float32:
                raise hip.Sc2Error('hyper_params_term: mode {!r} takes the f32 params'.format(self.encoder_precision))
            return self._precise_conv(params_nhwc, 'ep1a', pk['C1p'], 1, 0, hip.EPI_BIAS, pk['eb1'], hip.OUT_F32_NHWC,
                                      'entropy_parameters.0.params')
        return hip.conv2d_fwd(params_nhwc, pk['ep1a'], pk['C1p'], 1, 1, 1, 0, epilogue=hip.EPI_BIAS, ep_beta=pk['eb1'],
                              out_format=hip.OUT_F32_NHWC, tag='entropy_parameters.0.params')

    def _scan_inputs(self, z_hat_nhwc):
        """-> (p1 f32 [B, H, W, C1p], y_hat_pad f32 zeros [B, H+2, W+4, M]) for the y grid of 4x z's size."""
        precise = self._precise_ns() is not None
        p1 = self.hyper_params_term(self.hyper_synthesis(z_hat_nhwc, out_format=hip.OUT_F32_NHWC if precise else hip.OUT_BF16_NHWC))
        B, H, W, _ = p1.shape
        y_hat_pad = torch.zeros((B, H + 2, W + 4, self.M), dtype=torch.float32, device=p1.device)
        return p1, y_hat_pad

    def _check_tables(self):
        gc = self.gaussian_conditional
        if gc.scale_table.numel() == 0 or gc._quantized_cdf.numel() == 0:
            raise ValueError('Uninitialized scale table. Run update() first')
        return gc

    def compress_device(self, x, gaussian_params=None):
        """-> dict(y, symbols, indexes [B, H*W*M] pixel-major, y_hat_pad, p1, z_strings, shape) with the scan done on the device."""
        gc = self._check_tables()
        y = self.analysis(x)
        z = self.hyper_analysis(y)
        z_strings = self.entropy_bottleneck.compress(z)
        p1, y_hat_pad = self._scan_inputs(self._z_hat_nhwc(z_strings, z.shape[-2:]))
        B, H, W, _ = p1.shape
        if tuple(y.shape[-2:]) != (H, W):
            raise ValueError('mbt2018: the latent is {} but its hyperprior covers {}: the input size must be a multiple of '
                             '{}'.format(tuple(y.shape[-2:]), (H, W), self.downsampling_factor))
        sym = torch.empty((B, H * W * self.M), dtype=torch.int32, device=y.device)
        idx = torch.empty_like(sym)
        hip.ar_scan(self._scan_weights(), p1, y_hat_pad, None, gc.scale_table.float().contiguous(), gc._scale_bound,
                    y=y.float().contiguous(), symbols=sym, indexes=idx, gaussian_params=gaussian_params)
        return {'y': y, 'symbols': sym, 'indexes': idx, 'y_hat_pad': y_hat_pad, 'p1': p1, 'z_strings': z_strings,
                'shape': z.size()[-2:]}

    def compress(self, x):
        out = self.compress_device(x)
        y_strings = _encode_strings(self.gaussian_conditional, out['symbols'], out['indexes'])
        return {'strings': [y_strings, out['z_strings']], 'shape': out['shape']}

    def decompress_device(self, strings, shape, gaussian_params=None, chunks=1):
        """-> (y_hat_pad f32 [B, H+2, W+4, M], y_hat bf16 NHWC [B, H, W, M], symbols [B, H*W*M]); raises on a corrupt stream.
        In the precise encoder modes y_hat is None: g_s takes the f32 interior of y_hat_pad, and the scan writes no bf16 copy.
        `chunks` > 1 splits the scan into that many launches over consecutive pixel ranges (the decoder state carries over)."""
        assert isinstance(strings, list) and len(strings) == 2
        gc = self._check_tables()
        p1, y_hat_pad = self._scan_inputs(self._z_hat_nhwc(strings[1], shape))
        B, H, W, _ = p1.shape
        if len(strings[0]) != B:
            raise ValueError('Invalid strings or shape: {} y strings for {} z strings'.format(len(strings[0]), B))
        dev = p1.device
        buf, off, nb = gc.pack_strings(strings[0], dev)
        cdf, cdf_len, offset = gc._tables()
        dec = {'buf': buf, 'off': off, 'nb': nb, 'cdfs': cdf, 'cdf_sizes': cdf_len.int().contiguous(),
               'offsets': offset.int().contiguous(), 'cdf_entries': int(cdf_len.sum().item()) - cdf_len.numel(),
               'st_x': torch.zeros(B, dtype=torch.int64, device=dev), 'st_pos': torch.zeros(B, dtype=torch.int32, device=dev),
               'status': torch.zeros(B, dtype=torch.int32, device=dev)}
        y_hat = torch.empty((B, H, W, self.M), dtype=torch.bfloat16, device=dev) if self._precise_ns() is None else None
        sym = torch.empty((B, H * W * self.M), dtype=torch.int32, device=dev)
        n = H * W
        bounds = [n * i // chunks for i in range(chunks + 1)]
        for i in range(chunks):
            hip.ar_scan(self._scan_weights(), p1, y_hat_pad, y_hat, gc.scale_table.float().contiguous(), gc._scale_bound,
                        symbols=sym, decode=dec, pix=(bounds[i], bounds[i + 1]), gaussian_params=gaussian_params)
        what = 'JointAutoregressiveHierarchicalPriors.decompress'
        _raise_on_status(dec['status'] & ~16, what)   # bit 4 (16): the scan's own end-of-stream check
        if int((dec['status'] & 16).max().item()):
            raise ValueError('{}: a byte stream does not end where its last symbol ends (corrupt or foreign stream)'.format(what))
        return y_hat_pad, y_hat, sym

    def decompress(self, strings, shape):
        y_hat_pad, y_hat, _ = self.decompress_device(strings, shape)
        if self._precise_ns() is not None:      # symbols + means is not bf16-exact: g_s takes the f32 y_hat
            y_hat = y_hat_pad[:, 2:, 2:y_hat_pad.shape[2] - 2, :].contiguous()
        return {'x_hat': self.synthesis_nhwc(y_hat).clamp_(0, 1)}


def _encode_strings(gc, sym, idx):
    """int32 symbols / indexes [B, n] on the device -> list[bytes], one rANS stream per row (the batched device coder)."""
    buf, off, nb, st = gc.encode_symbols_device(sym, idx)
    if int(st.max().item()) != 0:
        buf, off, nb, st = gc.encode_symbols_device(sym, idx, out_stride=hip.rans_max_bytes(sym.shape[1]))
        _raise_on_status(st, 'GaussianConditional.compress')
    nb_h = nb.cpu().numpy()
    stride = buf.shape[1]
    width = int(nb_h.max())
    tail = buf[:, stride - width:].contiguous().cpu().numpy()
    return [tail[i, width - int(nb_h[i]):].tobytes() for i in range(tail.shape[0])]


# compressai.zoo.image [recalled]: quality -> (N, M)
HYPERPRIOR_CFGS = {q: ((128, 192) if q <= 5 else (192, 320)) for q in range(1, 9)}
MEAN_SCALE_CFGS = {q: ((128, 192) if q <= 4 else (192, 320)) for q in range(1, 9)}
MBT2018_CFGS = {q: ((192, 192) if q <= 4 else (192, 320)) for q in range(1, 9)}


def _zoo_model(zoo_name, file_stem, cls, cfgs, quality, metric, pretrained, kwargs):
    import logging
    import os
    import warnings
    if metric not in ('mse', 'ms-ssim'):
        raise ValueError('Invalid metric "{}"'.format(metric))
    if quality < 1 or quality > 8:
        raise ValueError('Invalid quality "{}", should be between (1, 8)'.format(quality))
    model = cls(*cfgs[quality], **kwargs)
    if pretrained:
        root = os.environ.get('SC2_PRETRAINED_DIR')
        path = os.path.join(root, '{}-{}-{}.pth'.format(file_stem, metric, quality)) if root else None
        if path and os.path.isfile(path):
            from .ckpt import _torch_load
            model.load_state_dict(_torch_load(path))
        else:
            msg = ('{}(quality={}, pretrained=True): no local weights ({}); the model is RANDOMLY '
                   'INITIALISED'.format(zoo_name, quality, path or 'SC2_PRETRAINED_DIR unset'))
            if os.environ.get('SC2_STRICT_WEIGHTS') == '1':
                raise FileNotFoundError(msg)
            warnings.warn(msg)
            logging.getLogger(__name__).warning(msg)
    return model


@register_compression_model_func
def bmshj2018_hyperprior(quality, metric='mse', pretrained=False, progress=True, **kwargs):
    """compressai.zoo.bmshj2018_hyperprior; offline weights from $SC2_PRETRAINED_DIR/bmshj2018-hyperprior-{metric}-{quality}.pth
    (as bmshj2018_factorized)."""
    return _zoo_model('bmshj2018_hyperprior', 'bmshj2018-hyperprior', ScaleHyperprior, HYPERPRIOR_CFGS, quality, metric,
                      pretrained, kwargs)


@register_compression_model_func
def mbt2018_mean(quality, metric='mse', pretrained=False, progress=True, **kwargs):
    """compressai.zoo.mbt2018_mean; offline weights from $SC2_PRETRAINED_DIR/mbt2018-mean-{metric}-{quality}.pth."""
    return _zoo_model('mbt2018_mean', 'mbt2018-mean', MeanScaleHyperprior, MEAN_SCALE_CFGS, quality, metric, pretrained, kwargs)


@register_compression_model_func
def mbt2018(quality, metric='mse', pretrained=False, progress=True, **kwargs):
    """compressai.zoo.mbt2018; offline weights from $SC2_PRETRAINED_DIR/mbt2018-{metric}-{quality}.pth."""
    return _zoo_model('mbt2018', 'mbt2018', JointAutoregressiveHierarchicalPriors, MBT2018_CFGS, quality, metric, pretrained,
                      kwargs)

def get_compression_model(compression_model_config, device):
    """sc2bench/models/registry.py:83-105: {'key', 'kwargs', 'src_ckpt'?, 'update'?} -> model on `device`, CDF tables
    built unless `update: False`."""
    if compression_model_config is None:
        return None
    name = compression_model_config['key']
    kwargs = compression_model_config.get('kwargs') or dict()
    ckpt_path = compression_model_config.get('src_ckpt', None)
    if name in COMPRESSION_MODEL_FUNC_DICT or name in COMPRESSION_MODEL_CLASS_DICT:
        builder = COMPRESSION_MODEL_FUNC_DICT.get(name) or COMPRESSION_MODEL_CLASS_DICT[name]
        model = builder(**kwargs)
        if ckpt_path is not None:
            from .ckpt import load_ckpt
            load_ckpt(ckpt_path, model=model, strict=None)
        if compression_model_config.get('update', True):
            model.update()
        return model.to(device)
    raise ValueError('compression_model_name `{}` is not expected'.format(name))
