"""Bottleneck layers: host-side mirror of sc2bench/models/layer.py for the hot path.

Same registry (`register_layer_class`, `LAYER_CLASS_DICT`, `get_layer`: layer.py:11-38, 820-835), same
class names, constructor arguments, module paths (`encoder`, `decoder`, `entropy_bottleneck`), methods
(`forward/encode/decode/update/aux_loss/_get_means/load_state_dict`) and mode switching
(layer.py:535-550) as the reference, so `bottleneck_config: {key: 'FPBasedResNetBottleneck', ...}` from
the reference's YAML files builds this class unchanged.  The arithmetic runs in libsc2amd.so: activations
stay bf16 NHWC between the implicit-GEMM kernels; GDN1 is a 1x1 MFMA GEMM with fused epilogue.
"""
import functools

import torch
from torch import nn

from . import hip
from .entropy import (CompressionModel, GDN1, GaussianConditional, HipConv2d, HipConvTranspose2d, _require_device,
                      get_scale_table, run_hip_sequence, run_hip_sequence_precise, update_registered_buffers)

LAYER_CLASS_DICT = dict()
LAYER_FUNC_DICT = dict()
_SPLIT_PARTS = {'bf16x3': 2, 'bf16x6': 3}   # encoder precision -> bf16 parts per operand (csrc/conv_split.hip)


def register_layer_class(cls):
    """Registers a layer class under its class name (layer.py:15-25)."""
    LAYER_CLASS_DICT[cls.__name__] = cls
    return cls


def register_layer_func(func):
    """Registers a function that builds a layer module (layer.py:28-38)."""
    LAYER_FUNC_DICT[func.__name__] = func
    return func


class EntropyBottleneckLayer(CompressionModel):
    """An entropy bottleneck as a stand-alone layer (layer.py:346-398)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.updated = False

    def forward(self, x):
        return self.entropy_bottleneck(x)

    def compress(self, x):
        strings = self.entropy_bottleneck.compress(x)
        return {'strings': [strings], 'shape': x.size()[-2:]}

    def decompress(self, strings, shape):
        assert isinstance(strings, list) and len(strings) == 1
        return self.entropy_bottleneck.decompress(strings[0], shape)

    def update(self, force=False):
        self.updated = True
        return super().update(force=force)


class BaseBottleneck(CompressionModel):
    """Abstract entropy-bottleneck-based layer (layer.py:401-441)."""

    def __init__(self, entropy_bottleneck_channels):
        super().__init__(entropy_bottleneck_channels=entropy_bottleneck_channels)
        self.updated = False

    def encode(self, *args, **kwargs):
        raise NotImplementedError()

    def decode(self, *args, **kwargs):
        raise NotImplementedError()

    def forward(self, *args):
        raise NotImplementedError()

    def update(self, force=False):
        self.updated = True
        return super().update(force=force)


@register_layer_class
class FPBasedResNetBottleneck(BaseBottleneck):
    """Factorized-prior encoder / entropy bottleneck / decoder for ResNet (layer.py:444-550).

    :param num_input_channels: number of input channels
    :param num_bottleneck_channels: number of bottleneck (latent) channels
    :param num_target_channels: number of output channels of the decoder
    :param encoder_channel_sizes: 4 channel counts of the encoder or None
    :param decoder_channel_sizes: 4 channel counts of the decoder or None

    ``output_format``: 'f32_nchw' (what the reference returns; default) or 'bf16_nhwc' (a bf16
    channels_last view, zero-copy input for a bf16 task head).
    """

    def __init__(self, num_input_channels=3, num_bottleneck_channels=24, num_target_channels=256,
                 encoder_channel_sizes=None, decoder_channel_sizes=None):
        if encoder_channel_sizes is None:
            encoder_channel_sizes = \
                [num_input_channels, num_bottleneck_channels * 4, num_bottleneck_channels * 2, num_bottleneck_channels]
        if decoder_channel_sizes is None:
            decoder_channel_sizes = \
                [encoder_channel_sizes[-1], num_target_channels * 2, num_target_channels, num_target_channels]
        super().__init__(entropy_bottleneck_channels=num_bottleneck_channels)
        e, d = encoder_channel_sizes, decoder_channel_sizes
        self.encoder = nn.Sequential(
            HipConv2d(e[0], e[1], kernel_size=5, stride=2, padding=2, bias=False),
            GDN1(e[1]),
            HipConv2d(e[1], e[2], kernel_size=5, stride=2, padding=2, bias=False),
            GDN1(e[2]),
            HipConv2d(e[2], e[3], kernel_size=2, stride=1, padding=0, bias=False)
        )
        self.decoder = nn.Sequential(
            HipConv2d(d[0], d[1], kernel_size=2, stride=1, padding=1, bias=False),
            GDN1(d[1], inverse=True),
            HipConv2d(d[1], d[2], kernel_size=2, stride=1, padding=0, bias=False),
            GDN1(d[2], inverse=True),
            HipConv2d(d[2], d[3], kernel_size=2, stride=1, padding=1, bias=False)
        )
        self._init_transforms()

    def _g_a(self):
        return self.encoder

    def _g_s(self):
        return self.decoder

    def _init_transforms(self):
        """Launch tags + pipeline switches shared by every bottleneck built on the FP analysis / synthesis stacks."""
        for prefix, seq in (('enc', self._g_a()), ('dec', self._g_s())):
            for i, mod in enumerate(seq):
                mod._tag = '{}.{}{}'.format(prefix, 'igdn' if getattr(mod, 'inverse', False) else
                                            'gdn' if isinstance(mod, GDN1) else 'conv', i)
        self.output_format = 'f32_nchw'
        self.fuse_gdn = True    # conv + GDN1 in one launch where one tile holds all output channels
        self.encoder_precision = 'bf16'   # 'f32': reference-precision analysis transform (set_encoder_precision)
        self.conv0_reads_nchw = True      # bf16 encoder: the first stage reads the f32 NCHW planes in place (False: A/B, layout pass)
        self._conv0_pack = None
        self._conv0_key = None

    # ---- fused pipelines on bf16 NHWC ---------------------------------------------------------- #
    def _conv0_packed(self):
        w = self._g_a()[0].weight
        key = (w._version, w.device, w.data_ptr())
        if self._conv0_key != key:
            self._conv0_pack = hip.pack_conv0_weight_pairs(w)
            self._conv0_key = key
        return self._conv0_pack

    def _gdn48_fragments(self, gamma_packed):
        """fragment-major form of the packed effective gamma [48][64] (cached per packed tensor)."""
        if getattr(self, '_g48_src', None) is not gamma_packed:
            self._g48_frag = hip.pack_weight_fragments(gamma_packed)
            self._g48_src = gamma_packed
        return self._g48_frag

    def _conv0_fragments(self):
        packed = self._conv0_packed()
        if getattr(self, '_conv0_frag_src', None) is not packed:
            self._conv0_frag = hip.pack_weight_fragments(packed[:self._g_a()[0].out_channels])
            self._conv0_frag_src = packed
        return self._conv0_frag

    def _uses_pair_conv0(self, x):
        c0 = self._g_a()[0]
        return (c0.in_channels <= 4 and c0.kernel_size == (5, 5) and c0.stride == (2, 2) and c0.padding == (2, 2)
                and c0.out_channels % 8 == 0)

    def set_encoder_precision(self, precision):
        """'bf16' (default): the analysis transform on the bf16 matrix cores -- fast, but ~1-2 % of the symbols of an image
        differ from the reference's f32 CPU path (a latent within bf16 rounding distance of a .5 boundary flips).
        'f32': f32 operands on the f32 matrix cores (csrc/conv_f32.hip; an exact f32 fma chain, 1/16 of the bf16 rate): the
        symbols -- hence the byte streams and bpp -- are the reference's up to the order of f32 additions (~1e-5 of the
        symbols).
        'bf16x3' / 'bf16x6': f32 activations and weights written as sums of two / three bf16 parts, the part products with index
        sum <= 1 / <= 2 (three / six per k) accumulated in f32 on the bf16 matrix cores (csrc/conv_split.hip).  Every product is
        exact, so the error is that of the dropped products: 'bf16x3' leaves 5e-6 of the symbols different from the f32 oracle
        (600 times fewer than 'bf16'), 'bf16x6' 6.5e-7, half of what 'f32' measures, at 0.72 / 0.91 of the time of 'f32'.  Use
        'bf16x3' when most images should code to the reference's bytes at a fraction of the cost of 'f32', 'bf16x6' when as
        many as possible should.  Measured times: DESIGN.md row g3.
        Only the encoder: the decoder's precision moves logits within tolerance, never a bitstream."""
        if precision not in ('bf16', 'f32') + tuple(_SPLIT_PARTS):
            raise ValueError("encoder precision must be 'bf16', 'f32', 'bf16x3' or 'bf16x6', got {!r}".format(precision))
        self.encoder_precision = precision
        return self

    set_compute_dtype = set_encoder_precision    # the bottleneck-level switch VERDICT r2 asks for, under that name

    def _f32_pack(self, mod, ns=0):
        """cached fragment-major operands of one analysis module: conv -> (weights, bias or None, padded Cin); GDN1 ->
        (effective gamma as a 1x1 conv, effective beta).  ns = 0: f32 (hip.pack_conv_f32); 2 / 3: bf16 parts (hip.pack_conv_split)."""
        cache = self.__dict__.setdefault('_f32_cache', {})
        pack = (lambda w: hip.pack_conv_split(w, ns)) if ns else hip.pack_conv_f32
        params = [q for q in (getattr(mod, 'weight', None), getattr(mod, 'bias', None), getattr(mod, 'beta', None),
                              getattr(mod, 'gamma', None)) if q is not None]
        key = tuple((q._version, q.data_ptr(), str(q.device)) for q in params)
        ent = cache.get((id(mod), ns))
        if ent is None or ent[0] != key:
            with torch.no_grad():
                if isinstance(mod, GDN1):
                    C = mod.in_channels
                    gamma = mod.gamma_reparam(mod.gamma).float().reshape(C, C, 1, 1)
                    ent = (key, pack(gamma), mod.beta_reparam(mod.beta).float().contiguous())
                else:
                    bias = None if mod.bias is None else mod.bias.detach().float().contiguous()
                    ent = (key, pack(mod.weight), bias)
            cache[(id(mod), ns)] = ent
        return ent[1], ent[2]

    def _analysis_f32(self, x, symbols_for=None, out=None, ns=0, slice_bytes=0x7FF00000 - 1):
        """encoder(x) with f32 operands (set_encoder_precision('f32')): every Conv2d / GDN1 of the analysis stack as one
        launch of sc2_conv2d_f32_fwd on f32 NHWC activations; the last conv writes the f32 NCHW latent or the symbols.
        ns = 2 / 3 ('bf16x3' / 'bf16x6'): the same walk on sc2_conv2d_split_fwd.  slice_bytes: the largest f32 tensor of a launch."""
        mods = list(self._g_a())
        if ns:
            conv, fused_ok, sfx = functools.partial(hip.conv2d_split_fwd, ns=ns), hip.conv_split_fused_gdn_supported, '.bf16x{}'.format(3 * (ns - 1))
        else:
            conv, fused_ok, sfx = hip.conv2d_f32_fwd, hip.conv_f32_fused_gdn_supported, '.f32'
        # sc2_conv2d_f32_fwd addresses activations through 32-bit buffer descriptors: every f32 tensor of a launch stays below
        # 2 GB (include/sc2_bottleneck.h).  The widest map of the stack is the first stage's output (C0 x H/2 x W/2 floats per
        # image: 4.8 MB at 224 x 224, i.e. ~445 images); larger batches run as slices of the batch
        if x.dim() == 4 and x.shape[0] > 1:
            per_image = 4 * max(x.shape[1] * x.shape[2] * x.shape[3],
                                max(getattr(m, 'out_channels', 0) for m in mods) * ((x.shape[2] + 1) // 2) * ((x.shape[3] + 1) // 2))
            n_max = max(1, slice_bytes // per_image)
            if x.shape[0] > n_max:
                parts = []
                flat = None if out is None else out.view(x.shape[0], -1)
                for i in range(0, x.shape[0], n_max):
                    parts.append(self._analysis_f32(x[i:i + n_max].contiguous(), symbols_for=symbols_for,
                                                    out=None if flat is None else flat[i:i + n_max], ns=ns, slice_bytes=slice_bytes))
                res = torch.cat(parts)
                return res if out is None else out.view(res.shape)
        # an RGB image goes to the first convolution as it is (f32 NCHW, three planes read in place); anything else as f32 NHWC
        rgb_in_place = (x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32 and x.is_contiguous() and
                        isinstance(mods[0], nn.Conv2d) and mods[0].in_channels == 3)
        h = x if rgb_in_place else hip.nchw_f32_to_nhwc_f32(x)
        fused_into_previous = False
        for i, mod in enumerate(mods):
            last = i == len(mods) - 1
            first_kw = dict(x_is_nchw_rgb=True) if (i == 0 and rgb_in_place) else {}
            if fused_into_previous:      # this GDN1 ran inside the conv before it
                fused_into_previous = False
                continue
            if isinstance(mod, GDN1):
                if type(mod) is not GDN1:
                    raise hip.Sc2Error('f32 analysis: {} is not supported'.format(type(mod).__name__))
                gamma, beta = self._f32_pack(mod, ns)
                h = conv(h, gamma, mod.in_channels, 1, 1, 1, 0, a_op=hip.AOP_ABS,
                         epilogue=hip.EPI_IGDN if mod.inverse else hip.EPI_GDN, ep_x=h, ep_beta=beta,
                         out_format=hip.OUT_F32_NCHW if last else hip.OUT_F32_NHWC, tag=mod._tag + sfx)
                continue
            if not isinstance(mod, nn.Conv2d) or mod.groups != 1 or mod.dilation != (1, 1) or mod.stride[0] != mod.stride[1] \
                    or mod.padding[0] != mod.padding[1]:
                raise hip.Sc2Error('f32 analysis: unsupported module {}'.format(mod))
            w, bias = self._f32_pack(mod, ns)
            kh, kw = mod.kernel_size
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if (self.fuse_gdn and type(nxt) is GDN1 and bias is None and nxt.in_channels == mod.out_channels <= 96 and
                    fused_ok(mod.out_channels) and i + 2 < len(mods)):
                # conv + GDN1 in one launch: the wave that owns a pixel's channels applies the normalisation to its accumulators
                gamma, beta = self._f32_pack(nxt, ns)
                h = conv(h, w, mod.out_channels, kh, kw, mod.stride, mod.padding,
                         epilogue=hip.EPI_FUSED_IGDN if nxt.inverse else hip.EPI_FUSED_GDN, ep_x=gamma, ep_beta=beta,
                         out_format=hip.OUT_F32_NHWC, tag=mod._tag + sfx + '+' + nxt._tag + sfx, cin_real=mod.in_channels, **first_kw)
                fused_into_previous = True
                continue
            if last and symbols_for is not None and bias is None:
                sym = conv(h, w, mod.out_channels, kh, kw, mod.stride, mod.padding, out_format=hip.OUT_I32_NCHW_SYM,
                           ep_beta=symbols_for._median_vector(), out=out, tag=mod._tag + sfx, cin_real=mod.in_channels, **first_kw)
                return sym
            h = conv(h, w, mod.out_channels, kh, kw, mod.stride, mod.padding,
                     epilogue=hip.EPI_NONE if bias is None else hip.EPI_BIAS, ep_beta=bias,
                     out_format=hip.OUT_F32_NCHW if last else hip.OUT_F32_NHWC, tag=mod._tag + sfx, cin_real=mod.in_channels, **first_kw)
        if symbols_for is None:
            return h
        sym = symbols_for.quantize(h, 'symbols', self._get_means(h))
        if out is not None:
            out.view(sym.shape).copy_(sym)
            return out.view(sym.shape)
        return sym

    def analysis(self, x, symbols_for=None, out=None):
        """encoder(x): f32 NCHW image batch -> f32 NCHW latent (layer.py:475-483).  `symbols_for` = an entropy model:
        the last conv then writes int32 symbols round(latent - median) directly (its epilogue quantises the f32
        accumulators; bit-identical to latent -> EntropyModel.quantize(.., 'symbols')) and the latent is never stored.
        `out` (with `symbols_for`): a contiguous int32 tensor of the symbols' element count to write them into."""
        _require_device(x, 'FPBasedResNetBottleneck')
        c0, g1, c2, g3, c4 = self._g_a()
        x = x.float()
        if self.encoder_precision == 'f32' or self.encoder_precision in _SPLIT_PARTS:
            return self._analysis_f32(x, symbols_for=symbols_for, out=out, ns=_SPLIT_PARTS.get(self.encoder_precision, 0))
        fuse0 = self.fuse_gdn and c0.out_channels in hip.FUSABLE_GDN_CHANNELS
        fuse2 = self.fuse_gdn and c2.out_channels in hip.FUSABLE_GDN_CHANNELS
        if self._uses_pair_conv0(x):
            N, _, H, W = x.shape
            in_place = (fuse0 and g1.in_channels == 96 and W % 2 == 0 and x.shape[1] == 3 and self.conv0_reads_nchw and
                        hip.conv0_gdn96_supported((N, H, W // 2, 8), c0.out_channels))
            if in_place:
                # the RGB batch goes to the first stage as it is (f32 NCHW, the reference's input layout): the kernel rounds the
                # three colour planes to bf16 as it stages them -- no layout launch, no [N,H,W,4] copy
                beta, gamma_f = g1.effective_fragments()
                h = hip.conv0_gdn96_nchw_fwd(x.contiguous(), self._conv0_fragments(), gamma_f, beta, g1.inverse,
                                             tag=c0._tag + '+' + g1._tag)
            else:
                if x.shape[-1] % 2:      # odd width (513): one zero column, exactly what the conv's own padding would read
                    x = torch.nn.functional.pad(x, (0, 1))
                    N, _, H, W = x.shape
                x4 = hip.nchw_f32_to_nhwc_bf16(x, 4, tag='enc.layout')    # [N,H,W,4]
                xp = x4.view(N, H, W // 2, 8)                             # pixel pairs
            if in_place:
                pass
            elif fuse0 and g1.in_channels == 96 and hip.conv0_gdn96_supported(tuple(xp.shape), c0.out_channels):
                beta, gamma_f = g1.effective_fragments()   # conv + GDN1(96) as one persistent streaming launch
                h = hip.conv0_gdn96_fwd(xp, self._conv0_fragments(), gamma_f, beta, g1.inverse,
                                        tag=c0._tag + '+' + g1._tag)
            elif fuse0:
                beta, gamma = g1.effective()
                h = hip.conv2d_fwd(xp, self._conv0_packed(), c0.out_channels, 5, 3, (2, 1), (2, 1),
                                   epilogue=hip.EPI_FUSED_IGDN if g1.inverse else hip.EPI_FUSED_GDN, ep_x=gamma,
                                   ep_beta=beta, tag=c0._tag + '+' + g1._tag)
            else:
                h = hip.conv2d_fwd(xp, self._conv0_packed(), c0.out_channels, 5, 3, (2, 1), (2, 1), tag=c0._tag)
        else:
            fuse0 = False
            cin = c0.in_channels
            xin = hip.nchw_f32_to_nhwc_bf16(x, (cin + 7) // 8 * 8)
            if cin % 8 != 0:
                w = torch.zeros((c0.out_channels, xin.shape[-1]) + tuple(c0.kernel_size), dtype=c0.weight.dtype,
                                device=c0.weight.device)
                w[:, :cin] = c0.weight.detach()
                h = hip.conv2d_fwd(xin, hip.pack_conv_weight(w), c0.out_channels, c0.kernel_size[0],
                                   c0.kernel_size[1], c0.stride, c0.padding)
            else:
                h = c0.forward_nhwc(xin)
        if not fuse0:
            h = g1.forward_nhwc(h)
        if fuse2 and g3.in_channels == 48 and hip.conv2_gdn48_supported(tuple(h.shape), c2.out_channels, c2.kernel_size[0],
                                                                        c2.kernel_size[1], c2.stride, c2.padding):
            beta, gamma = g3.effective()   # conv + GDN1(48) as one persistent launch, weights resident in registers
            h = hip.conv2_gdn48_fwd(h, c2.packed_weight(hip.K_SLAB_MAJOR | hip.K_B_FRAG_MAJOR), self._gdn48_fragments(gamma),
                                    beta, g3.inverse, tag=c2._tag + '+' + g3._tag)
        elif fuse2:
            beta, gamma = g3.effective()
            epi = hip.EPI_FUSED_IGDN if g3.inverse else hip.EPI_FUSED_GDN
            order = c2.k_order()
            if hip.conv_patch_supported(tuple(h.shape), c2.out_channels, c2.kernel_size[0], c2.kernel_size[1], c2.stride,
                                        c2.padding, epilogue=epi):
                order = hip.K_SLAB_MAJOR | hip.K_B_FRAG_MAJOR   # input patch staged in LDS once (conv5s2_patch_kernel)
            h = hip.conv2d_fwd(h, c2.packed_weight(order), c2.out_channels, c2.kernel_size[0], c2.kernel_size[1],
                               c2.stride, c2.padding, epilogue=epi, ep_x=gamma, ep_beta=beta,
                               tag=c2._tag + '+' + g3._tag, k_order=order)
        else:
            h = g3.forward_nhwc(c2.forward_nhwc(h))
        if c4.bias is None and hip.conv2x2_c48_supported(tuple(h.shape), c4.out_channels, c4.kernel_size[0], c4.kernel_size[1],
                                                         c4.stride, c4.padding):
            # the streaming form of encoder[4] (48 -> 24, k2): f32 latent, or the coder's symbols straight from the accumulators
            key = (c4.weight._version, c4.weight.device, c4.weight.data_ptr())
            if getattr(self, '_c48_key', None) != key:
                with torch.no_grad():
                    self._c48_frag = hip.pack_conv2x2_c48(c4.weight)
                self._c48_key = key
            med = symbols_for._median_vector() if symbols_for is not None else None
            return hip.conv2x2_c48_fwd(h, self._c48_frag, c4.out_channels, medians=med, tag=c4._tag,
                                       out=out if symbols_for is not None else None)
        if symbols_for is not None and c4.bias is None and c4.out_channels <= 96 and c4.out_channels % 8 == 0:
            sym = hip.conv2d_fwd(h, c4.packed_weight(), c4.out_channels, c4.kernel_size[0], c4.kernel_size[1], c4.stride,
                                 c4.padding, out_format=hip.OUT_I32_NCHW_SYM, ep_beta=symbols_for._median_vector(),
                                 tag=c4._tag, k_order=c4.k_order())
        else:
            latent = c4.forward_nhwc(h, out_format=hip.OUT_F32_NCHW)
            if symbols_for is None:
                return latent
            sym = symbols_for.quantize(latent, 'symbols', self._get_means(latent))
        if out is not None:
            out.view(sym.shape).copy_(sym)
            return out.view(sym.shape)
        return sym

    def synthesis_nhwc_tail(self, y_hat_nhwc, head):
        """decoder on a bf16 NHWC latent WITH the first two 1x1 layers of the HIP task head `head` (layer2.0's conv1 and
        downsample) fused behind its last conv: -> (None, (conv1 output, downsample output)) for `HipHead.forward(pre=...)`, or
        (decoder output, None) when the geometry is not the 224 x 224 operating point, or None when `head` has no such
        block.  In the fused case the decoder's own output is never materialised."""
        spec = head.tail_spec()
        c4 = self._g_s()[4]
        if spec is None or c4.bias is not None or tuple(c4.kernel_size) != (2, 2) or c4.out_channels != 256:
            return None
        h = self.synthesis_nhwc(y_hat_nhwc, upto_last=True)
        if not hip.conv2x2_win_tail_supported(tuple(h.shape)) or tuple(c4.padding) != (1, 1):
            return self._last_conv(h), None
        # keyed on the tensors that are packed (their storage and version), not on the identity of `head`: a rebuilt
        # HipHead may reuse the address of a dropped one
        key = tuple((t.data_ptr(), t._version, str(t.device)) for t in (c4.weight,) + tuple(spec))
        cache = self.__dict__.setdefault('_tail_cache', {})
        if cache.get('key') != key:
            w1, b1, wds, bds = spec
            with torch.no_grad():
                cache['val'] = (hip.pack_conv2x2_win_tail(c4.weight.detach(), w1, wds), b1, bds)
            cache['key'] = key
        stream, b1, bds = cache['val']
        o1, ods, _ = hip.conv2x2_win_tail_fwd(h, stream, b1, bds, tag=c4._tag + '+head.2.0')
        return None, (o1, ods)

    def _last_conv(self, h):
        c4 = self._g_s()[4]
        if self.output_format == 'bf16_nhwc':
            if c4.bias is None and hip.conv2x2_win_supported(tuple(h.shape), c4.out_channels, c4.kernel_size[0], c4.kernel_size[1],
                                                             c4.stride, c4.padding):
                out = hip.conv2x2_win_fwd(h, self._win_weights(c4, None)[1], c4.padding[0], tag=c4._tag)
            else:
                out = c4.forward_nhwc(h, out_format=hip.OUT_BF16_NHWC)
            return out.permute(0, 3, 1, 2)  # logical NCHW, channels_last memory
        return c4.forward_nhwc(h, out_format=hip.OUT_F32_NCHW)

    def synthesis_nhwc(self, y_hat_nhwc, upto_last=False):
        """decoder on a bf16 NHWC latent (layer.py:485-493); output per ``self.output_format``."""
        c0, g1, c2, g3, c4 = self._g_s()
        if (self.fuse_gdn and g1.in_channels == c0.out_channels and
                hip.conv2x2_gdn512_supported(c0.in_channels, c0.out_channels, c0.kernel_size[0], c0.kernel_size[1],
                                             c0.stride, c0.padding)):
            beta, gamma = g1.effective_fragments()   # conv + (inverse) GDN1(512) in one persistent launch
            h = hip.conv2x2_gdn512_fwd(y_hat_nhwc, c0.packed_weight(hip.K_TAP_MAJOR), gamma, beta, g1.inverse, tag=c0._tag + '+' + g1._tag)
        else:
            h = c0.forward_nhwc(y_hat_nhwc)
            h = g1.forward_nhwc(h)
        fused = hip.conv_fused_gdn_supported(tuple(h.shape), c2.out_channels, c2.kernel_size[0], c2.kernel_size[1],
                                             c2.stride, c2.padding) if self.fuse_gdn else 0
        win2 = (self.fuse_gdn and type(g3) is GDN1 and g3.in_channels == c2.out_channels == 256 and c2.bias is None and
                hip.conv2x2_win_supported(tuple(h.shape), c2.out_channels, c2.kernel_size[0], c2.kernel_size[1], c2.stride,
                                          c2.padding))
        if win2:
            # conv + inverse GDN1 on the window-plane kernel (bit-identical to the tile kernel's fused launch)
            beta, w_frag = self._win_weights(c2, g3)
            h = hip.conv2x2_win_fwd(h, w_frag, c2.padding[0], beta=beta, inverse=g3.inverse, tag=c2._tag + '+' + g3._tag)
        elif fused:
            # conv + inverse GDN1 in one launch (256-wide big tile holds all channels)
            beta, gamma = g3.effective_fragments() if fused == 2 else g3.effective()
            h = hip.conv2d_fwd(h, c2.packed_weight(), c2.out_channels, c2.kernel_size[0], c2.kernel_size[1], c2.stride,
                               c2.padding, epilogue=hip.EPI_FUSED_IGDN if g3.inverse else hip.EPI_FUSED_GDN,
                               ep_x=gamma, ep_beta=beta, tag=c2._tag + '+' + g3._tag, k_order=c2.k_order())
        else:
            h = c2.forward_nhwc(h)
            h = g3.forward_nhwc(h)
        if upto_last:
            return h
        return self._last_conv(h)

    def _win_weights(self, conv, gdn):
        """(beta, weight stream) of sc2_conv2x2_win_fwd for `conv` [+ the GDN1 behind it]; cached per parameter version."""
        key = (conv.weight._version, conv.weight.device, conv.weight.data_ptr()) + \
            (() if gdn is None else (gdn.beta._version, gdn.gamma._version, gdn.gamma.data_ptr()))
        cache = self.__dict__.setdefault('_win_cache', {})
        ent = cache.get(id(conv))
        if ent is None or ent[0] != key:
            with torch.no_grad():
                if gdn is None:
                    ent = (key, None, hip.pack_conv2x2_win(conv.weight))
                else:
                    beta = gdn.beta_reparam(gdn.beta).float().contiguous()
                    ent = (key, beta, hip.pack_conv2x2_win(conv.weight, gdn.gamma_reparam(gdn.gamma)))
            cache[id(conv)] = ent
        return ent[1], ent[2]

    def synthesis(self, y_hat):
        """decoder(y_hat) for an f32 NCHW latent."""
        _require_device(y_hat, 'FPBasedResNetBottleneck')
        return self.synthesis_nhwc(hip.nchw_f32_to_nhwc_bf16(y_hat.float(), y_hat.shape[1]))

    # ---- reference API -------------------------------------------------------------------------- #
    def encode(self, x, **kwargs):
        """-> {'strings': [list of N byte strings], 'shape': latent spatial size} (layer.py:496-507)."""
        eb = self.entropy_bottleneck
        eb._tables()     # "Uninitialized CDFs. Run update() first" before any device work
        # the last encoder conv quantises its own accumulators (round(acc - median)): the coder's symbols without an f32 latent
        sym = self.analysis(x, symbols_for=eb)
        shape = torch.Size(sym.shape[-2:])
        latent_strings = eb.compress_symbols(sym.reshape(sym.shape[0], -1), shape[0] * shape[1])
        return {'strings': [latent_strings], 'shape': shape}

    def decode(self, strings, shape):
        """strings, shape -> decoder output (layer.py:509-521)."""
        _, y_hat_nhwc = self.entropy_bottleneck.decompress_to_device(strings[0], tuple(shape), want_f32=False, want_nhwc=True)
        return self.synthesis_nhwc(y_hat_nhwc)

    def encode_device(self, x):
        """Device-resident encode: (buf, offset, nbytes, status, latent spatial size); no host sync."""
        latent = self.analysis(x)
        buf, off, nb, st = self.entropy_bottleneck.compress_device(latent)
        return buf, off, nb, st, tuple(latent.shape[-2:])

    def decode_device(self, buf, off, nb, shape):
        _, y_hat_nhwc = self.entropy_bottleneck.decompress_device(buf, off, nb, tuple(shape), want_f32=False,
                                                                  want_nhwc=True)
        return self.synthesis_nhwc(y_hat_nhwc)

    # ---- the eval forward (encode -> bytes -> decode) cut into stages for `pipeline.StagePipeline`: the serial range coder
    #      of several batches then shares one launch on its own HIP stream while the MFMA streams work on neighbouring batches
    stage_front_takes_out = True     # stage_front(x, out=): the last encoder conv writes the coder's symbols into `out` itself
    stage_coder_kwargs = {'dequantized': True}   # what a pipeline passes to stage_coder (plain calls return the int32 symbols)

    def stage_front(self, x, out=None):
        """encoder + quantisation (layer.py:496-506 up to the coder): -> (symbols int32 [N, C*h*w], (h, w)).  `out`: a contiguous
        int32 [N, C*h*w] tensor to write the symbols into (a row block of the buffer one range-coder launch will read)."""
        sym = self.analysis(x, symbols_for=self.entropy_bottleneck, out=out)
        return sym.view(sym.shape[0], -1), tuple(sym.shape[-2:])

    def stage_coder(self, sym, hw_shape, dequantized=False):
        """rANS encode to byte streams, then decode them (layer.py:506 + :520): -> (decoded, nbytes [N], status [N]).
        `dequantized`: `decoded` is the dequantised latent as bf16 NHWC [N, h, w, C] (decode + EntropyModel.dequantize in one
        coder launch, the int32 symbols are never written) when the tables allow it, else the int32 symbols."""
        eb = self.entropy_bottleneck
        hw = hw_shape[0] * hw_shape[1]
        buf, off, nb, st = eb.encode_symbols_device(sym, hw)
        if dequantized:
            y_hat = eb.decode_dequantize_device(buf, off, nb, sym.shape[1], hw_shape)
            if y_hat is not None:
                return y_hat, nb, st
        dec = eb.decode_symbols_device(buf, off, nb, sym.shape[1], hw)
        return dec, nb, st

    def stage_coder_host(self, sym, hw_shape, dequantized=False, staging=None, slot=0, d2h_event=None):
        """`stage_coder` on the host thread pool (EntropyBottleneck.code_on_host): the same streams, coded by CPU cores -- a batch of
        256 serial chains takes 64 cores ~3 ms where the device's lanes take ~21 ms, which is what the FIRST batches of a pipelined
        run wait for (pipeline.StagePipeline `host_steps`).  Returns what `stage_coder(..., dequantized=True)` returns."""
        return self.entropy_bottleneck.code_on_host(sym, hw_shape, staging=staging, slot=slot, d2h_event=d2h_event)

    def stage_decode(self, decoded, hw_shape):
        """what `stage_coder` returned -> the dequantised latent, bf16 NHWC (the input of `synthesis_nhwc`)."""
        if decoded.dtype == torch.bfloat16:
            return decoded
        return self.entropy_bottleneck.dequantize_device(decoded, hw_shape)[1]

    def _get_means(self, x):
        medians = self.entropy_bottleneck._get_medians().detach()
        spatial_dims = len(x.size()) - 2
        medians = self.entropy_bottleneck._extend_ndims(medians, spatial_dims)
        return medians.expand(x.size(0), *([-1] * (spatial_dims + 1)))

    def _needs_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _forward2train(self, x):
        if self._needs_grad(x):
            from .autograd import bottleneck_forward2train_autograd
            return bottleneck_forward2train_autograd(self, x)
        encoded_obj = self.analysis(x)
        y_hat, y_likelihoods = self.entropy_bottleneck(encoded_obj)
        return self.synthesis(y_hat)

    def forward(self, x):
        # if fine-tune or evaluate after "update"
        if self.updated:
            if not self.training:
                encoded_obj = self.encode(x)
                decoded_obj = self.decode(**encoded_obj)
                return decoded_obj
            if self._needs_grad(x):
                from .autograd import bottleneck_forward_updated_autograd
                return bottleneck_forward_updated_autograd(self, x)
            encoded_output = self.analysis(x)
            decoder_input = self.entropy_bottleneck.dequantize(
                self.entropy_bottleneck.quantize(encoded_output, 'dequantize', self._get_means(encoded_output)))
            decoder_input = decoder_input.detach()
            return self.synthesis(decoder_input)
        return self._forward2train(x)


def _hyper_transform(seq):
    """nn.Conv2d / nn.ConvTranspose2d (bias-free) of a user-supplied h_a / h_s -> their HIP-backed subclasses in place
    (same parameters, same state-dict keys)."""
    for i, m in enumerate(seq):
        if type(m) is nn.Conv2d and m.bias is None and m.groups == 1 and m.dilation == (1, 1):
            c = HipConv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, bias=False)
            c.weight = m.weight
            seq[i] = c
        elif type(m) is nn.ConvTranspose2d and m.bias is None and m.groups == 1 and m.dilation == (1, 1) and \
                m.output_padding == (0, 0):
            c = HipConvTranspose2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, bias=False)
            c.weight = m.weight
            seq[i] = c
    return seq


@register_layer_class
class SHPBasedResNetBottleneck(BaseBottleneck):
    """Scale-hyperprior encoder / hyper-codec / decoder for ResNet (layer.py:553-720).

    g_a / g_s are the FP bottleneck's analysis / synthesis stacks (same fused kernels); h_a / h_s run on the
    implicit-GEMM kernel (transposed convolutions as stride-parity classes); the latent y is coded with the
    Gaussian conditional model whose per-element CDF rows come from h_s(z_hat), z with the factorised prior.

    :param num_input_channels: number of input channels
    :param num_latent_channels: number of latent (hyper) channels
    :param num_bottleneck_channels: number of bottleneck channels
    :param num_target_channels: number of output channels of the decoder
    :param h_a: parametric transform h_a or None
    :param h_s: parametric transform h_s or None
    :param g_a_channel_sizes: 4 channel counts of g_a or None
    :param g_s_channel_sizes: 4 channel counts of g_s or None
    """

    def __init__(self, num_input_channels=3, num_latent_channels=16, num_bottleneck_channels=24,
                 num_target_channels=256, h_a=None, h_s=None, g_a_channel_sizes=None, g_s_channel_sizes=None):
        if g_a_channel_sizes is None:
            g_a_channel_sizes = \
                [num_input_channels, num_bottleneck_channels * 4, num_bottleneck_channels * 2, num_bottleneck_channels]
        else:
            num_bottleneck_channels = g_a_channel_sizes[3]
        if g_s_channel_sizes is None:
            g_s_channel_sizes = \
                [g_a_channel_sizes[-1], num_target_channels * 2, num_target_channels, num_target_channels]
        super().__init__(entropy_bottleneck_channels=num_latent_channels)
        a, g = g_a_channel_sizes, g_s_channel_sizes
        self.g_a = nn.Sequential(
            HipConv2d(a[0], a[1], kernel_size=5, stride=2, padding=2, bias=False),
            GDN1(a[1]),
            HipConv2d(a[1], a[2], kernel_size=5, stride=2, padding=2, bias=False),
            GDN1(a[2]),
            HipConv2d(a[2], a[3], kernel_size=2, stride=1, padding=0, bias=False)
        )
        self.g_s = nn.Sequential(
            HipConv2d(g[0], g[1], kernel_size=2, stride=1, padding=1, bias=False),
            GDN1(g[1], inverse=True),
            HipConv2d(g[1], g[2], kernel_size=2, stride=1, padding=0, bias=False),
            GDN1(g[2], inverse=True),
            HipConv2d(g[2], g[3], kernel_size=2, stride=1, padding=1, bias=False)
        )
        L, B = num_latent_channels, num_bottleneck_channels
        self.h_a = nn.Sequential(
            HipConv2d(B, L, kernel_size=5, stride=2, padding=1, bias=False),
            nn.ReLU(inplace=True),
            HipConv2d(L, L, kernel_size=5, stride=2, padding=2, bias=False)
        ) if h_a is None else _hyper_transform(h_a)
        self.h_s = nn.Sequential(
            HipConvTranspose2d(L, L, kernel_size=5, stride=2, padding=1, bias=False),
            nn.LeakyReLU(inplace=True),
            HipConvTranspose2d(L, L, kernel_size=5, stride=2, padding=1, bias=False),
            nn.LeakyReLU(inplace=True),
            HipConv2d(L, B, kernel_size=5, stride=1, padding=0, bias=False)
        ) if h_s is None else _hyper_transform(h_s)
        self.gaussian_conditional = GaussianConditional(None)
        self.num_latent_channels = num_latent_channels
        self.num_bottleneck_channels = num_bottleneck_channels
        self._init_transforms()
        for prefix, seq in (('h_a', self.h_a), ('h_s', self.h_s)):
            for i, mod in enumerate(seq):
                mod._tag = '{}.{}'.format(prefix, i)

    # the FP bottleneck's fused analysis / synthesis pipelines, on g_a / g_s
    _g_a = lambda self: self.g_a        # noqa: E731
    _g_s = lambda self: self.g_s        # noqa: E731
    _init_transforms = FPBasedResNetBottleneck._init_transforms
    _conv0_packed = FPBasedResNetBottleneck._conv0_packed
    _conv0_fragments = FPBasedResNetBottleneck._conv0_fragments
    _gdn48_fragments = FPBasedResNetBottleneck._gdn48_fragments
    _uses_pair_conv0 = FPBasedResNetBottleneck._uses_pair_conv0
    analysis = FPBasedResNetBottleneck.analysis
    synthesis_nhwc = FPBasedResNetBottleneck.synthesis_nhwc
    _win_weights = FPBasedResNetBottleneck._win_weights
    synthesis_nhwc_tail = FPBasedResNetBottleneck.synthesis_nhwc_tail
    _last_conv = FPBasedResNetBottleneck._last_conv
    synthesis = FPBasedResNetBottleneck.synthesis
    _f32_pack = FPBasedResNetBottleneck._f32_pack
    _analysis_f32 = FPBasedResNetBottleneck._analysis_f32
    _hyper_abs = True       # h_a sees |y| (layer.py:641,675)

    def set_encoder_precision(self, precision):
        """The FP bottleneck's switch ('bf16' default, 'f32', 'bf16x3', 'bf16x6': FPBasedResNetBottleneck.set_encoder_precision),
        here a property of the CODEC, not only of the encoder.  Three floating-point transforms decide the bytes of a hyperprior
        stream: g_a the y symbols, h_a the z symbols, and h_s the CDF-row index of every y symbol (and MSHP's means) -- which the
        DECODER rebuilds from the decoded z.  In the three precise modes all of them run on the precise kernels (csrc/conv_f32.hip /
        conv_split.hip; the transposed convolutions of h_s as stride-parity classes, activations in the f32 epilogue, the
        hyper-latent travelling as f32) in every no-grad path: encode, decode, the eval and updated-train forward, the likelihood
        path without grad, stage_front / stage_coder.  g_s, the autograd training paths and 'bf16' are what they were.
        A stream made in one mode is only guaranteed to decode in THAT mode: another mode's h_s may put a scale on the other side
        of a scale-table boundary, and one wrong index desynchronises the range decoder.  Set the same mode on both ends."""
        return FPBasedResNetBottleneck.set_encoder_precision(self, precision)

    set_compute_dtype = set_encoder_precision

    def _precise_ns(self):
        """None in 'bf16' mode, else the bf16 parts per operand of the precise kernels (0: f32 operands)."""
        if self.encoder_precision == 'bf16':
            return None
        return _SPLIT_PARTS.get(self.encoder_precision, 0)

    # ---- hyper transforms on the device --------------------------------------------------------- #
    def hyper_analysis(self, y):
        """z = h_a(|y|) (SHP) or h_a(y) (MSHP): f32 NCHW latent -> f32 NCHW hyper-latent."""
        a_op = hip.AOP_ABS if self._hyper_abs else hip.AOP_NONE
        ns = self._precise_ns()
        if ns is not None:
            return run_hip_sequence_precise(self.h_a, hip.nchw_f32_to_nhwc_f32(y.float()), ns, a_op=a_op)
        y_nhwc = hip.nchw_f32_to_nhwc_bf16(y.float().contiguous(), y.shape[1])
        return run_hip_sequence(self.h_a, y_nhwc, a_op=a_op)

    def hyper_synthesis(self, z_hat_nhwc):
        """h_s(z_hat) on an NHWC hyper-latent (bf16; f32 in the precise modes: what _z_hat_nhwc / _z_hat_from_symbols return)
        -> f32 NCHW Gaussian parameters."""
        ns = self._precise_ns()
        if ns is not None:
            if z_hat_nhwc.dtype != torch.float32:
                raise hip.Sc2Error('hyper_synthesis: mode {!r} takes the f32 hyper-latent'.format(self.encoder_precision))
            return run_hip_sequence_precise(self.h_s, z_hat_nhwc, ns)
        return run_hip_sequence(self.h_s, z_hat_nhwc)

    def _z_hat_nhwc(self, z_hat):
        if self._precise_ns() is not None:      # symbols + medians is not bf16-exact: the hyper-latent stays f32
            return hip.nchw_f32_to_nhwc_f32(z_hat.float())
        return hip.nchw_f32_to_nhwc_bf16(z_hat.float().contiguous(), z_hat.shape[1])

    def _z_hat_from_symbols(self, z_sym, z_shape):
        """int32 z symbols [N, L*hz*wz] -> the dequantised hyper-latent as hyper_synthesis takes it."""
        eb = self.entropy_bottleneck
        if self._precise_ns() is not None:
            return self._z_hat_nhwc(eb.dequantize_device(z_sym, tuple(z_shape), want_f32=True, want_nhwc=False)[0])
        return eb.dequantize_device(z_sym, tuple(z_shape), want_f32=False, want_nhwc=True)[1]

    def _params(self, gaussian_params):
        """-> (scales_hat, means_hat or None)"""
        return gaussian_params, None

    # ---- reference API -------------------------------------------------------------------------- #
    def encode(self, x, **kwargs):
        """-> {'strings': [y_strings, z_strings], 'shape': z spatial size} (layer.py:630-648 / 765-777)."""
        y = self.analysis(x)
        z = self.hyper_analysis(y)
        z_shape = z.size()[-2:]
        eb = self.entropy_bottleneck
        # the coder is lossless: z_hat = dequantize(symbols) is what decompress(compress(z)) returns (layer.py:643-645), so the
        # hyper-synthesis does not wait for the serial coder; both streams are then coded by whichever coder suits the batch
        z_sym = eb.symbols_device(z)
        scales_hat, means_hat = self._params(self.hyper_synthesis(self._z_hat_from_symbols(z_sym, z_shape)))
        indices = self.gaussian_conditional.build_indexes(scales_hat)
        y_strings = self.gaussian_conditional.compress(y, indices, means=means_hat)
        z_strings = eb.compress_symbols(z_sym, int(z_shape[0]) * int(z_shape[1]))
        return {'strings': [y_strings, z_strings], 'shape': z_shape}

    def decode(self, strings, shape):
        """strings [y_strings, z_strings], z shape -> decoder output (layer.py:650-666 / 779-786)."""
        assert isinstance(strings, list) and len(strings) == 2
        eb = self.entropy_bottleneck
        dev = eb._quantized_cdf.device
        if dev.type != 'cuda':
            raise hip.Sc2Error('{}.decode: module is on {}; HIP device required'.format(type(self).__name__, dev))
        if self._precise_ns() is not None:     # the SAME mode as the encoder's: its h_s decides the indexes
            z_hat_nhwc = self._z_hat_nhwc(eb.decompress_to_device(strings[1], tuple(shape), want_f32=True, want_nhwc=False)[0])
        else:
            _, z_hat_nhwc = eb.decompress_to_device(strings[1], tuple(shape), want_f32=False, want_nhwc=True)
        scales_hat, means_hat = self._params(self.hyper_synthesis(z_hat_nhwc))
        indices = self.gaussian_conditional.build_indexes(scales_hat)
        _, y_hat_nhwc = self.gaussian_conditional.decompress_to_device(strings[0], indices, means_hat, want_f32=False,
                                                                       want_nhwc=True)
        return self.synthesis_nhwc(y_hat_nhwc)

    # ---- the same eval forward in stages (pipeline.StagePipeline)
    stage_front_takes_out = False
    stage_coder_kwargs = {}

    def stage_front(self, x, out=None):
        """encode() up to the coders (layer.py:630-647 / 765-776): g_a, h_a, the hyper-latent's symbols, the Gaussian parameters
        from its dequantised form, and in ONE pass the latent's symbols and their CDF-row indexes:
        -> ((y symbols [N, C*h*w], indexes [N, C*h*w], z symbols [N, L*hz*wz]), ((h, w), (hz, wz)))."""
        y = self.analysis(x)
        z = self.hyper_analysis(y)
        eb, gc = self.entropy_bottleneck, self.gaussian_conditional
        z_shape = tuple(z.shape[-2:])
        z_sym = eb.symbols_device(z)
        scales_hat, means_hat = self._params(self.hyper_synthesis(self._z_hat_from_symbols(z_sym, z_shape)))
        y_sym, idx = gc.symbols_indexes_device(y, scales_hat, means_hat)
        N = y.shape[0]
        return (y_sym.view(N, -1), idx.view(N, -1), z_sym), (tuple(y.shape[-2:]), z_shape)

    def stage_coder(self, payload, meta):
        """Both byte streams of every image are produced (layer.py:646-647) and then decoded as decode() decodes them
        (layer.py:650-666 / 779-786): z from ITS bytes, the Gaussian parameters from the decoded z, the indexes from those, y
        from its bytes with these indexes: -> (y_hat bf16 NHWC [N, h, w, C], nbytes of both streams [N], status [N])."""
        y_sym, idx, z_sym = payload
        (h, w), (hz, wz) = meta
        eb, gc = self.entropy_bottleneck, self.gaussian_conditional
        N = y_sym.shape[0]
        zb, zo, znb, zst = eb.encode_symbols_device(z_sym, hz * wz)
        yb, yo, ynb, yst = gc.encode_symbols_device(y_sym, idx)
        z_dec = eb.decode_symbols_device(zb, zo, znb, z_sym.shape[1], hz * wz)
        scales_hat, means_hat = self._params(self.hyper_synthesis(self._z_hat_from_symbols(z_dec, (hz, wz))))
        idx2 = gc.build_indexes(scales_hat)
        y_dec, dst = gc.decode_symbols_device(yb, yo, ynb, idx2.view(N, -1))
        C = y_sym.shape[1] // (h * w)
        _, y_hat_nhwc = hip.gc_dequantize(y_dec.view(N, C, h, w), None if means_hat is None else means_hat.float(),
                                          want_f32=False, want_nhwc=True)
        return y_hat_nhwc, ynb + znb, yst | zst | dst

    def stage_decode(self, decoded, meta):
        return decoded

    def _get_means(self, x):
        medians = self.entropy_bottleneck._get_medians().detach()
        spatial_dims = len(x.size()) - 2
        medians = self.entropy_bottleneck._extend_ndims(medians, spatial_dims)
        return medians.expand(x.size(0), *([-1] * (spatial_dims + 1)))

    _needs_grad = FPBasedResNetBottleneck._needs_grad

    def _forward2train(self, x):
        if self._needs_grad(x):
            from .autograd import hyperprior_forward2train_autograd
            return hyperprior_forward2train_autograd(self, x)
        y = self.analysis(x)
        z = self.hyper_analysis(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales_hat, means_hat = self._params(self.hyper_synthesis(self._z_hat_nhwc(z_hat)))
        y_hat, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        self.last_likelihoods = (y_likelihoods, z_likelihoods)
        return self.synthesis(y_hat)

    def forward(self, x):
        # if fine-tune or evaluate after "update"
        if self.updated:
            if not self.training:
                encoded_obj = self.encode(x)
                decoded_obj = self.decode(**encoded_obj)
                return decoded_obj
            with torch.no_grad():
                y = self.analysis(x)
                y_hat = self.gaussian_conditional.dequantize(
                    self.gaussian_conditional.quantize(y, 'dequantize', self._get_means(y))
                )
            y_hat = y_hat.detach()
            return self._synthesis_maybe_grad(x, y_hat)
        return self._forward2train(x)

    def _synthesis_maybe_grad(self, x, y_hat):
        if self._needs_grad(x):
            from .autograd import synthesis_autograd
            return synthesis_autograd(self, y_hat)
        return self.synthesis(y_hat)

    def update(self, scale_table=None, force=False):
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        updated |= super().update(force=force)
        self.updated = True
        return updated

    def load_state_dict(self, state_dict, **kwargs):
        """Resizes the registered buffers of the Gaussian model to the checkpoint's shapes, then loads
        (layer.py:706-720)."""
        update_registered_buffers(self.gaussian_conditional, 'gaussian_conditional',
                                  ['_quantized_cdf', '_offset', '_cdf_length', 'scale_table'], state_dict)
        return super().load_state_dict(state_dict, **kwargs)


@register_layer_class
class MSHPBasedResNetBottleneck(SHPBasedResNetBottleneck):
    """Mean-scale-hyperprior encoder / hyper-codec / decoder for ResNet (layer.py:723-817)."""
    _hyper_abs = False      # h_a sees y itself (layer.py:767,789)

    def __init__(self, num_input_channels=3, num_latent_channels=16, num_bottleneck_channels=24,
                 num_target_channels=256, g_a_channel_sizes=None, g_s_channel_sizes=None):
        L, B = num_latent_channels, num_bottleneck_channels
        h_a = nn.Sequential(
            HipConv2d(B, L, kernel_size=5, stride=2, padding=1, bias=False),
            nn.LeakyReLU(inplace=True),
            HipConv2d(L, L, kernel_size=5, stride=2, padding=2, bias=False)
        )
        h_s = nn.Sequential(
            HipConvTranspose2d(L, L, kernel_size=5, stride=2, padding=1, bias=False),
            nn.LeakyReLU(inplace=True),
            HipConvTranspose2d(L, L * 3 // 2, kernel_size=5, stride=2, padding=1, bias=False),
            nn.LeakyReLU(inplace=True),
            HipConv2d(L * 3 // 2, B * 2, kernel_size=5, stride=1, padding=0, bias=False)
        )
        super().__init__(num_input_channels=num_input_channels, num_latent_channels=num_latent_channels,
                         num_bottleneck_channels=num_bottleneck_channels, num_target_channels=num_target_channels,
                         h_a=h_a, h_s=h_s, g_a_channel_sizes=g_a_channel_sizes, g_s_channel_sizes=g_s_channel_sizes)

    def _params(self, gaussian_params):
        scales_hat, means_hat = gaussian_params.chunk(2, 1)
        return scales_hat, means_hat

    def forward(self, x):
        # if fine-tune or evaluate after "update"
        if self.updated:
            if not self.training:
                encoded_obj = self.encode(x)
                decoded_obj = self.decode(**encoded_obj)
                return decoded_obj
            with torch.no_grad():
                y = self.analysis(x)
                z = self.hyper_analysis(y)
                z_hat = self.entropy_bottleneck.dequantize(
                    self.entropy_bottleneck.quantize(z, 'dequantize', self._get_means(z))
                )
                scales_hat, means_hat = self._params(self.hyper_synthesis(self._z_hat_nhwc(z_hat)))
                y_hat = self.gaussian_conditional.dequantize(
                    self.gaussian_conditional.quantize(y, 'dequantize', means_hat)
                )
            y_hat = y_hat.detach()
            return self._synthesis_maybe_grad(x, y_hat)
        return self._forward2train(x)


# ------------------------------------------------------------------------------------------------------------------ CR+BQ
def _bn_affine(bn):
    """eval-mode BatchNorm2d as y = a * x + b: (a, b) f32 [C]"""
    var, mean = bn.running_var.detach().float(), bn.running_mean.detach().float()
    gamma = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(var)
    a = gamma * torch.rsqrt(var + bn.eps)
    return a.contiguous(), (beta - mean * a).contiguous()


def _pad_dim(t, dim, size):
    if t.shape[dim] == size:
        return t
    shape = list(t.shape)
    shape[dim] = size - t.shape[dim]
    return torch.cat([t, t.new_zeros(shape)], dim)


def _sole_transform(module, cls):
    """`module` if it is a `cls`, the member of a one-transform `Compose` if that is one, else None"""
    if isinstance(module, cls):
        return module
    members = getattr(module, 'transforms', None)
    if isinstance(members, (list, tuple)) and len(members) == 1 and isinstance(members[0], cls):
        return members[0]
    return None


# the module sequence of `larger_resnet_bottleneck`: (type, (in, out, kernel, stride, padding) of a conv) -- None: the bottleneck width
_BQ_SEQUENCE = (('conv', (3, 64, 7, 2, 3)), ('bn', 64), ('relu',), ('maxpool',), ('bn', 64), ('relu',),
                ('conv', (64, None, 2, 2, 1)), ('bn', None), ('relu',),
                ('conv', (None, 512, 2, 1, 1)), ('bn', 512), ('relu',), ('conv', (512, 512, 2, 1, 1)), ('bn', 512), ('relu',),
                ('conv', (512, 512, 2, 1, 0)), ('bn', 512), ('relu',), ('conv', (512, 512, 2, 1, 0)), ('avgpool',))


class _BqHipPlan(object):
    """Eval-mode `larger_resnet_bottleneck` on the library's kernels: every BatchNorm2d folded into the convolution in front of
    it (bf16 weights, f32 bias, ReLU in the epilogue) except the two that follow no convolution -- the one behind the max-pool
    (`hip.maxpool_affine_relu_nhwc`) and, for bottleneck_idx 7, the decoder's first (`hip.bq_dequantize`'s affine)."""

    def __init__(self, mods, idx, channels):
        from .head import ConvSpec, _Conv
        self.idx, self.channels = idx, channels
        self.cpad = (channels + 7) // 8 * 8
        w = _pad_dim(mods[0].weight.detach().float(), 1, 8)       # 3 input channels -> 8 (zeros): 16-byte channel runs
        self.stem = _Conv(ConvSpec(w, mods[0].stride, mods[0].padding), mods[1], 'bq.stem')
        mp = mods[3]
        self.pool = (mp.kernel_size, mp.stride, mp.padding)
        self.pool_affine = _bn_affine(mods[4])
        # the bottleneck convolution: output channels zero-padded to a multiple of 8 (the kernels' granularity); its norm layer
        # belongs to the encoder only when bottleneck_idx is 9
        w = mods[6].weight.detach().float()
        bias = torch.zeros(self.cpad, dtype=torch.float32, device=w.device)
        if idx == 9:
            a, b = _bn_affine(mods[7])
            w = w * a.reshape(-1, 1, 1, 1)
            bias[:channels] = b
        self.conv_z = _Conv(ConvSpec(_pad_dim(w, 0, self.cpad), mods[6].stride, mods[6].padding), None, 'bq.conv_z')
        self.conv_z.b = bias
        self.dq_affine = _bn_affine(mods[7]) if idx == 7 else None
        w = _pad_dim(mods[9].weight.detach().float(), 1, self.cpad)
        self.dec = [_Conv(ConvSpec(w, mods[9].stride, mods[9].padding), mods[10], 'bq.dec0'),
                    _Conv(mods[12], mods[13], 'bq.dec1'), _Conv(mods[15], mods[16], 'bq.dec2'), _Conv(mods[18], None, 'bq.dec3')]
        ap = mods[19]
        self.avgpool = (int(ap.kernel_size if isinstance(ap.kernel_size, int) else ap.kernel_size[0]),
                        int(ap.stride if isinstance(ap.stride, int) else ap.stride[0]))

    def analysis(self, x):
        """f32 NCHW images -> the latent the compressor sees: f32 [N, channels, h, w]"""
        h = hip.nchw_f32_to_nhwc_bf16(x.float().contiguous(), 8, tag='bq.layout')
        h = self.stem(h, hip.EPI_BIAS_RELU)
        h = hip.maxpool_affine_relu_nhwc(h, self.pool_affine[0], self.pool_affine[1], *self.pool, tag='bq.pool')
        c = self.conv_z
        z = hip.conv2d_fwd(h, c.w, c.cout, c.k[0], c.k[1], c.stride, c.pad, epilogue=hip.EPI_BIAS_RELU if self.idx == 9 else hip.EPI_NONE,
                           ep_beta=c.b, out_format=hip.OUT_F32_NCHW, tag=c.tag, k_order=c.k_order)
        return z if self.cpad == self.channels else z[:, :self.channels].contiguous()

    def synthesis(self, q_x, output_format):
        """QuantizedTensor (u8 codes on the device) -> decoder output: bf16 [N, 512, H, W] as a view of NHWC memory, or f32 NCHW"""
        h = hip.bq_dequantize(q_x.tensor, q_x.scale, q_x.zero_point, out_format=hip.OUT_BF16_NHWC, affine=self.dq_affine,
                              relu=self.idx == 7, cpad=self.cpad)
        for conv in self.dec[:3]:
            h = conv(h, hip.EPI_BIAS_RELU)
        h = self.dec[3](h, hip.EPI_NONE)
        h = hip.avgpool2d_nhwc(h, self.avgpool[0], self.avgpool[1], tag='bq.avgpool')
        if output_format == 'bf16_nhwc':
            return h.permute(0, 3, 1, 2)
        return hip.nhwc_bf16_to_nchw_f32(h)


class SimpleBottleneck(nn.Module):
    """Encoder / decoder pair whose encoder output is the bottleneck (layer.py:41-105): encoder -> compressor (if given) ->
    decompressor (if given) -> decoder in eval mode, encoder -> decoder in training mode.

    A `larger_resnet_bottleneck` split at 7 or 9 with at most 16 bottleneck channels runs its eval forward on a device tensor
    on the library's kernels (`analysis`, `_BqHipPlan`); every other geometry, training mode, grad mode and CPU tensors run the
    torch modules.  `output_format` ('f32_nchw' | 'bf16_nhwc', set by the backbone's `set_compute_dtype`) is what `decode`
    hands to the task head on a device tensor in eval mode."""

    def __init__(self, encoder, decoder, compressor=None, decompressor=None):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.compressor = compressor
        self.decompressor = decompressor
        self.output_format = 'f32_nchw'
        self.bottleneck_idx = None      # set by the builders whose module sequence the HIP path knows
        self._bq_plan = None

    def _hip_geometry(self):
        """(modules, idx, channels) when encoder + decoder are `larger_resnet_bottleneck`'s sequence in eval mode split at 7 / 9"""
        idx = self.bottleneck_idx
        if idx not in (7, 9) or not isinstance(self.encoder, nn.Sequential) or not isinstance(self.decoder, nn.Sequential):
            return None
        mods = list(self.encoder) + list(self.decoder)
        if len(self.encoder) != idx or len(mods) != len(_BQ_SEQUENCE):
            return None
        channels = mods[6].out_channels if isinstance(mods[6], nn.Conv2d) else 0
        if not 0 < channels <= 16:
            return None
        for m, want in zip(mods, _BQ_SEQUENCE):
            if want[0] == 'conv':
                geo = tuple(channels if v is None else v for v in want[1])
                if not (type(m) is nn.Conv2d and m.bias is None and m.groups == 1 and m.dilation == (1, 1) and
                        (m.in_channels, m.out_channels) == geo[:2] and m.kernel_size == (geo[2],) * 2 and
                        m.stride == (geo[3],) * 2 and m.padding == (geo[4],) * 2):
                    return None
            elif want[0] == 'bn':
                if not (type(m) is nn.BatchNorm2d and not m.training and m.track_running_stats and m.running_mean is not None and
                        m.num_features == (channels if want[1] is None else want[1])):
                    return None
            elif want[0] == 'relu':
                if type(m) is not nn.ReLU:
                    return None
            elif want[0] == 'maxpool':
                if not (type(m) is nn.MaxPool2d and m.dilation in (1, (1, 1)) and not m.ceil_mode and not m.return_indices):
                    return None
            elif not (type(m) is nn.AvgPool2d and m.padding in (0, (0, 0)) and not m.ceil_mode and m.divisor_override is None and
                      m.kernel_size in (2, (2, 2)) and m.stride in (1, (1, 1))):
                return None
        return mods, idx, channels

    def _hip_plan(self, x):
        """the folded HIP form for this call, or None: eval mode without grad on a device tensor, a known geometry"""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and not self.training and not torch.is_grad_enabled()):
            return None
        geometry = self._hip_geometry()
        if geometry is None:
            return None
        # rebuilt when a parameter or buffer changes: in place (its version) or replaced (its address), as SplittableResNet's head
        tensors = list(self.encoder.parameters()) + list(self.encoder.buffers()) + list(self.decoder.parameters()) + \
            list(self.decoder.buffers())
        key = tuple((t._version, t.data_ptr()) for t in tensors) + (geometry[1], str(x.device))
        if self._bq_plan is None or self._bq_plan[0] != key:
            with torch.inference_mode(False), torch.no_grad():
                self._bq_plan = (key, _BqHipPlan(*geometry))
        return self._bq_plan[1]

    def analysis(self, x):
        """the encoder's output, in front of the compressor"""
        plan = self._hip_plan(x)
        return plan.analysis(x) if plan is not None else self.encoder(x)

    def encode(self, x):
        z = self.analysis(x)
        if self.compressor is not None:
            z = self.compressor(z)
        return {'z': z}

    def decode(self, z):
        from .transforms import QuantizedTensor, SimpleDequantizer
        codes = z.tensor if isinstance(z, QuantizedTensor) else None
        plan = self._hip_plan(codes) if codes is not None and codes.dtype == torch.uint8 else None
        dequantizer = _sole_transform(self.decompressor, SimpleDequantizer) if plan is not None else None
        if dequantizer is not None and dequantizer.num_bits != 16 and codes.dim() == 4 and codes.shape[1] == plan.channels:
            return plan.synthesis(z, self.output_format)
        if self.decompressor is not None:
            z = self.decompressor(z)
        y = self.decoder(z)
        if self.output_format == 'bf16_nhwc' and y.is_cuda and not self.training and not torch.is_grad_enabled():
            y = y.to(dtype=torch.bfloat16, memory_format=torch.channels_last)     # what the bf16 task head takes
        return y

    def forward(self, x):
        if not self.training:
            return self.decode(**self.encode(x))
        return self.decoder(self.encoder(x))

    def update(self):
        """nothing to update: this layer has no entropy model (kept for the callers that update every bottleneck)"""
        import logging
        logging.getLogger(__name__).info('This module has no updatable parameters for entropy coding')

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_bq_plan'] = None          # packed device weights of a cache do not belong in a pickle
        return state


@register_layer_func
def larger_resnet_bottleneck(bottleneck_channel=12, bottleneck_idx=7, compressor_transform=None, decompressor_transform=None):
    """ResNet-50/-101/-152 compatible bottleneck of Matsubara et al.'s head network distillation (layer.py:108-153): 20 modules,
    the first `bottleneck_idx` of them the encoder.  Same signature as the reference (its `ghnd-bq` configs pass an
    `output_channel` this builder does not take, and fail with the same TypeError here)."""
    width = bottleneck_channel

    def conv(cin, cout, stride=1, padding=0, kernel=2):
        return nn.Conv2d(cin, cout, kernel_size=kernel, stride=stride, padding=padding, bias=False)

    def norm_relu(c):
        return [nn.BatchNorm2d(c), nn.ReLU(inplace=True)]

    stack = [conv(3, 64, stride=2, padding=3, kernel=7)] + norm_relu(64)
    stack += [nn.MaxPool2d(kernel_size=3, stride=2, padding=1)] + norm_relu(64)
    stack += [conv(64, width, stride=2, padding=1)] + norm_relu(width)
    stack += [conv(width, 512, padding=1)] + norm_relu(512)
    stack += [conv(512, 512, padding=1)] + norm_relu(512)
    stack += [conv(512, 512)] + norm_relu(512)
    stack += [conv(512, 512), nn.AvgPool2d(kernel_size=2, stride=1)]
    layer = SimpleBottleneck(nn.Sequential(*stack[:bottleneck_idx]), nn.Sequential(*stack[bottleneck_idx:]),
                             compressor_transform, decompressor_transform)
    layer.bottleneck_idx = bottleneck_idx
    return layer


def get_layer(cls_or_func_name, **kwargs):
    """Gets a layer module by registered class or function name (layer.py:820-835)."""
    if cls_or_func_name in LAYER_CLASS_DICT:
        return LAYER_CLASS_DICT[cls_or_func_name](**kwargs)
    elif cls_or_func_name in LAYER_FUNC_DICT:
        return LAYER_FUNC_DICT[cls_or_func_name](**kwargs)
    return None
