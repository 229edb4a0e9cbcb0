"""Inference-time ResNet task head (layer2..fc) on the library's implicit-GEMM kernel.

The caller on the far side of the bottleneck path (reference: sc2bench/models/backbone.py:235-254, torchvision
Bottleneck blocks).  In eval mode BatchNorm is an affine map, so each conv+BN(+ReLU)(+residual) is ONE
`sc2_conv2d_fwd` launch: BN folded into the packed bf16 weights and a per-channel f32 bias, ReLU and the
residual add fused in the epilogue (SC2_EPI_BIAS / BIAS_RELU / BIAS_ADD_RELU).  Activations stay bf16 NHWC from
the decoder's output to the pooled features; the classifier is the same kernel as a 1x1 conv.

Only used when the model is in eval mode; training keeps the torch modules (BatchNorm statistics).
"""
import os

import torch
from torch import nn

from . import hip
from .resnet import Bottleneck, FrozenBatchNorm2d


def _fold(conv, bn):
    """conv (no bias) followed by an eval-mode norm layer -> (packed bf16 weight, f32 bias)."""
    w = conv.weight.detach().float()
    if bn is None:      # a bare convolution (the data-gradient convs of frozen.py): identity scale, zero bias
        scale = torch.ones(w.shape[0], dtype=torch.float32, device=w.device)
        bias = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
    elif isinstance(bn, (nn.BatchNorm2d, FrozenBatchNorm2d)):
        gamma = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(bn.running_mean)
        beta = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(bn.running_mean)
        scale = gamma * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
        bias = beta - bn.running_mean.detach().float() * scale
    else:
        raise TypeError('cannot fold {}'.format(type(bn)))
    w = w * scale.reshape(-1, 1, 1, 1)
    order = hip.preferred_k_order(w.shape[1], w.shape[2], w.shape[3])
    return hip.pack_conv_weight(w, order), bias.contiguous(), order, w


def _win1_policy(cin, cout, stride):
    """Which 1x1 layers go to the window-plane 1x1 kernel (conv1x1_win.hip).  SC2_CONV1X1_WIN: '0' none, 'all' every supported
    layer (A/B, tools/head_times.py), default = the layers it measured faster on."""
    mode = str(hip.host_policy.conv1x1_win)
    if mode == '0':
        return False
    if mode == 'all':
        return True
    # measured at bs 256, 224 x 224 (tools/head_times.py, SC2_CONV1X1_WIN=all against the default):
    #   conv1 of layer2.1-3 (512 -> 128)      0.075 -> 0.065 ms (streaming kernel)
    #   conv1 of layer4.1-2 (2048 -> 512)     0.064 -> 0.045 ms (tile kernel)
    #   conv3 of layer4     (512 -> 2048)     0.062 -> 0.054 ms (streaming kernel)
    #   downsample of layer3 (512 -> 1024 s2) 0.111 -> 0.101 ms (streaming kernel)
    # every other 1x1 layer was as fast or faster where it is (conv3 of layer2 / layer3 are HBM-bound: 0.104 -> 0.125 ms here)
    return (cin, cout, stride) in ((512, 128, 1), (2048, 512, 1), (512, 2048, 1), (512, 1024, 2))


# (cin, cout, stride) of the layers the eight-wave 256-channel 1x1 kernel (conv1x1_w8.hip) takes by default: the tuples it was faster on
# in EVERY one of five alternating rounds at bs 256, 224 x 224 (tools/head_times.py --w8-ab, profiles/r13_head_times_w8_ab.txt; ms per
# launch, the five rounds' range):
#   conv1 of layer3.1-5     (1024 -> 256)      0.0454 - 0.0460 -> 0.0416 - 0.0422   (from conv1x1_kres)
#   conv1 of layer4.0       (1024 -> 512)      0.0796 - 0.0808 -> 0.0703 - 0.0710   (from conv1x1_kres)
#   downsample of layer4    (1024 -> 2048 s2)  0.0815 - 0.0829 -> 0.0671 - 0.0676   (from conv1x1_kres)
#   downsample of layer3    (512 -> 1024 s2)   0.1014 - 0.1029 -> 0.0812 - 0.0829   (from conv1x1_win)
#   conv3 of layer4.0-2     (512 -> 2048)      0.0530 - 0.0539 -> 0.0478 - 0.0484   (from conv1x1_win)
# stays where it is: conv1 of layer4.1-2 (2048 -> 512: 112 whole tiles on 256 CUs) 0.0434 - 0.0444 -> 0.0588 - 0.0593; and, outside the
# kernel's brief but supported by it, conv3 of layer3 (256 -> 1024, HBM-bound) 0.0612 -> 0.0633 and layer2's downsample (256 -> 512 s2).
_W8_TABLE = ((1024, 256, 1), (1024, 512, 1), (1024, 2048, 2), (512, 1024, 2), (512, 2048, 1))


def _w8_policy(cin, cout, stride):
    """Which 1x1 layers go to the eight-wave 256-channel 1x1 kernel (conv1x1_w8.hip), asked at every call.
    hip.configure(conv1x1_w8=...) / bench.py --policy conv1x1_w8=...: '0' none, 'all' every supported layer (A/B, tools/head_times.py
    --w8-ab), default '1' = the layers it measured faster on in every round."""
    mode = str(hip.host_policy.conv1x1_w8)
    if mode in ('0', 'False'):
        return False
    if mode == 'all':
        return True
    return (cin, cout, stride) in _W8_TABLE


class ConvSpec(object):
    """What `_Conv` reads of an nn.Conv2d, for convolutions that exist only as a weight tensor."""
    bias = None
    groups = 1

    def __init__(self, weight, stride=(1, 1), padding=(0, 0), dilation=(1, 1)):
        self.weight = weight
        self.out_channels, self.in_channels = int(weight.shape[0]), int(weight.shape[1])
        self.kernel_size = (int(weight.shape[2]), int(weight.shape[3]))
        self.stride, self.padding, self.dilation = tuple(stride), tuple(padding), tuple(dilation)


class _Conv(object):
    """One folded conv + norm layer launch: `route` says which kernel a call takes, `__call__` makes that launch."""

    def __init__(self, conv, bn, tag):
        assert conv.bias is None and conv.groups == 1
        w_tile, self.b, self.k_order, w_folded = _fold(conv, bn)
        self.w_folded = w_folded       # f32 OIHW with the norm layer's scale folded in (frozen.py builds the data gradient from it)
        self.cin, self.cout = conv.in_channels, conv.out_channels
        self.k = conv.kernel_size
        self.stride = conv.stride
        self.pad = conv.padding
        self.dilation = conv.dilation
        self.tag = tag
        self.w2d = w_folded.reshape(w_folded.shape[0], w_folded.shape[1]).to(torch.bfloat16) if self.k == (1, 1) else None
        self._packed = {'tile': w_tile}      # the packed weight by layout: see `packed`
        geom = (self.cin, self.cout, self.k[0], self.k[1], self.stride, self.pad)
        undilated = self.dilation == (1, 1) or self.k == (1, 1)
        # The routes this layer is OPEN to, by its shape and the policy in force now (`route` lists which switch is read when).
        # HBM-bound 1x1 layers with a short K and a wide N: the persistent streaming kernel
        self.stream = hip.conv1x1_stream_supported(*geom) and undilated
        # K = 1024 / 2048 1x1 layers (conv1 of layer3 / layer4, layer4's downsample): weights resident in registers, one channel
        # chunk per workgroup
        self.kres = (not self.stream) and undilated and hip.conv1x1_kres_supported(*geom)
        # long-K 1x1 layers that are not HBM-bound: the window-plane 1x1 kernel (which layers: _win1_policy, by measurement)
        self.win1 = self.k == (1, 1) and _win1_policy(self.cin, self.cout, self.stride[0]) and hip.conv1x1_win_supported(*geom)
        # long-K 1x1 layers that are plain compute-heavy GEMMs: the eight-wave 256-channel kernel, on conv1x1_win's weight stream (not
        # the bare data-gradient convolutions of frozen.py: the gradient paths stay where they are).  WHICH of these layers it runs is
        # asked per call (_w8_policy), so hip.configure(conv1x1_w8=...) works on a built head
        self.w8_ok = bn is not None and self.k == (1, 1) and hip.conv1x1_w8_supported(*geom)
        # 3x3 stride-1 layers on 28 / 14 / 7 pixel maps and stride-2 layers on 56 / 28 / 14 pixel maps (conv2 of every block at the
        # 224 x 224 operating point): the window-plane kernel; other map sizes stay on the implicit-GEMM tile kernel (decided per call,
        # by the map size; 14 x 14 is a supported map of both the stride-1 and the stride-2 form)
        self.win3 = hip.conv3x3_win_supported(14, 14, *geom, self.dilation)
        # Dilated 3x3 layers (DeepLab's layer3 / layer4, torchvision `replace_stride_with_dilation`): sc2_conv2d_fwd takes the dilation
        # itself -- one launch on the generic tile with runtime dilation -- whenever the layer has more than 96 output channels;
        # narrower layers run as phase grids (`_phase_grids`)
        self.native_dilation = self.dilation != (1, 1) and self.k != (1, 1) and hip.weight_rows(self.cout) % 128 == 0
        if self.dilation != (1, 1) and not self.native_dilation:
            d = self.dilation[0]
            ok = (self.k == (3, 3) and self.stride == (1, 1) and self.dilation == (d, d) and self.pad == (d, d)) or self.k == (1, 1)
            if not ok:
                raise hip.Sc2Error('the HIP head supports dilation on layers of <= 96 output channels only as 3x3 stride-1 with '
                                   'padding == dilation (got kernel {}, stride {}, padding {}, dilation {})'.format(
                                       self.k, self.stride, self.pad, self.dilation))
        # Packed here: the layouts of the routes open now, so that no first call -- which may be inside a graph capture -- packs.  A
        # layer that hip.configure(conv1x1_w8=...) switches in later packs at its first call, as does conv1 of a pair launch (HipHead)
        if self.stream or self.kres:
            self.packed('frag')
        if self.win1 or self.win3 or (self.w8_ok and _w8_policy(self.cin, self.cout, self.stride[0])):
            self.packed('win')

    _PACKERS = {'tile': lambda c: hip.pack_conv_weight(c.w_folded, c.k_order),       # the implicit-GEMM tile kernel (sc2_conv2d_fwd)
                'frag': lambda c: hip.pack_weight_fragments(c.w_folded.reshape(c.cout, c.cin)),   # 1x1: stream, kres, the pair launch
                'win': lambda c: hip.pack_conv_win(c.w_folded)}                       # the window-plane kernels (win1, w8, win3)

    def packed(self, layout):
        """The folded weight in `layout` ('tile' / 'frag' / 'win'), packed once and kept: one device copy per layout and layer."""
        w = self._packed.get(layout)
        if w is None:
            w = self._packed[layout] = self._PACKERS[layout](self)
        return w

    w = property(lambda self: self._packed['tile'])

    def route(self, x_shape, epilogue, has_ep_x=False, has_mask=False):
        """The launch a call with these operands takes: the first name in the order below whose condition holds.  No tensor, no launch.

        plain calls    w8 > win1 > stream > kres > win3 > tile
        dilated 3x3    tile_dilated > phase_grids
        masked calls   win1_mask > stream_mask > win3_mask > mask_unfused      (ep_mask: the ReLU gradient behind a data gradient)

        Switches read when the layer is BUILT, through the flags they set (`stream`, `kres`, `win1`, `win3`): conv_stream, conv_kres,
        conv1x1_win, and conv_win / conv_win_s2 for whether the layer is open to win3 at all.  hip.configure() of these reaches only
        layers built afterwards.
        Switches read at EVERY call: conv1x1_w8 (_w8_policy), conv_win / conv_win_s2 (hip.conv3x3_win_supported, with the map size),
        relu_mask_fused, conv_dilation; and, in HipHead.forward, conv1x1_pair.

        Kept as they were, oddities included: the 32-bit operand bound covers input and output for w8 / win1 (the output counted at
        the INPUT's map size) but only the input for win3; kres takes no residual, hence no EPI_BIAS_ADD_RELU; w8 is closed to bare
        convolutions (`w8_ok`: bn is None); the masked win3 form needs stride 1 and no ep_x, and a layer open to stream or kres is not
        asked for it."""
        N, H, W, C = x_shape
        n_in, n_out, s = N * H * W * C, N * H * W * self.cout, self.stride[0]
        if has_mask:
            if hip.host_policy.relu_mask_fused and self.dilation == (1, 1) and hip._fits32(n_in, n_out):
                if self.win1:
                    return 'win1_mask'
                if self.stream and hip.conv1x1_stream_mask_supported(C, self.cout, s):
                    return 'stream_mask'
                if not has_ep_x and not (self.stream or self.kres) and self.win3 and self.stride == (1, 1) and \
                        hip.conv3x3_win_supported(H, W, C, self.cout, self.k[0], self.k[1], self.stride, self.pad):
                    return 'win3_mask'
            return 'mask_unfused'
        if self.dilation != (1, 1) and self.k != (1, 1):
            return 'tile_dilated' if self.native_dilation and hip.host_policy.conv_dilation else 'phase_grids'   # ('0': A/B)
        no_add = epilogue == hip.EPI_BIAS or epilogue == hip.EPI_BIAS_RELU
        fusable = no_add or epilogue == hip.EPI_BIAS_ADD_RELU
        if self.w8_ok and fusable and _w8_policy(self.cin, self.cout, s) and hip._fits32(n_in, n_out):
            return 'w8'
        if self.win1 and fusable and hip._fits32(n_in, n_out):
            return 'win1'
        if self.stream and fusable:
            return 'stream'
        if self.kres and no_add:
            return 'kres'
        if self.win3 and no_add and hip._fits32(n_in) and \
                hip.conv3x3_win_supported(H, W, C, self.cout, self.k[0], self.k[1], self.stride, self.pad):
            return 'win3'
        return 'tile'

    # the fused kernels by route name: (hip's launcher -- looked up at the call: tests and tools replace it --, weight layout, takes a
    # residual, takes a mask)
    _FUSED = {'w8': ('conv1x1_w8_fwd', 'win', True, False), 'kres': ('conv1x1_kres_fwd', 'frag', False, False),
              'win1': ('conv1x1_win_fwd', 'win', True, True), 'win1_mask': ('conv1x1_win_fwd', 'win', True, True),
              'stream': ('conv1x1_stream_fwd', 'frag', True, True), 'stream_mask': ('conv1x1_stream_fwd', 'frag', True, True),
              'win3': ('conv3x3_win_fwd', 'win', False, True), 'win3_mask': ('conv3x3_win_fwd', 'win', False, True)}

    def __call__(self, x, epilogue, ep_x=None, ep_mask=None):
        """ep_mask (bf16 like the output, epilogue EPI_BIAS): y = ep_mask > 0 ? conv + bias [+ ep_x] : 0 -- the ReLU gradient behind a
        data gradient (frozen.py; ep_x: a second gradient that reaches the same tensor, the skip path's, added in front of the mask);
        in the launch's epilogue on the window-plane and streaming kernels, else as a `relu_bwd` pass behind the unmasked launch."""
        assert ep_mask is None or epilogue == hip.EPI_BIAS
        name = self.route(x.shape, epilogue, ep_x is not None, ep_mask is not None)
        if name == 'mask_unfused':
            return hip.relu_bwd(self(x, epilogue), ep_mask, add=ep_x)
        if name == 'phase_grids':
            assert ep_x is None
            return self._phase_grids(x, epilogue)
        if name == 'tile' or name == 'tile_dilated':      # (a dilated 1x1 layer is an undilated one: 'tile' passes no dilation)
            return hip.conv2d_fwd(x, self.w, self.cout, self.k[0], self.k[1], self.stride, self.pad, epilogue=epilogue, ep_x=ep_x,
                                  ep_beta=self.b, tag=self.tag, k_order=self.k_order,
                                  dilation=self.dilation if name == 'tile_dilated' else 1)
        # (epilogue, ep_x, ep_mask) in the fused kernels' terms; a route that takes no residual or no mask is chosen only without one
        launcher, layout, takes_residual, takes_mask = self._FUSED[name]
        kw = {}
        if takes_residual:
            kw['residual'] = ep_x if ep_mask is not None or epilogue == hip.EPI_BIAS_ADD_RELU else None
        if takes_mask:
            kw['mask'] = ep_mask
        return getattr(hip, launcher)(x, self.packed(layout), self.b, stride=self.stride[0], relu=epilogue != hip.EPI_BIAS, tag=self.tag,
                                      **kw)

    def _phase_grids(self, x, epilogue):
        """a stride-1 conv with dilation d and padding d is d*d independent UNDILATED pad-1 convs on the phase grids x[a::d, b::d] --
        the same weights, the same kernel, outputs scattered back to y[a::d, b::d]"""
        d = self.dilation[0]
        N, H, W, _ = x.shape
        y = torch.empty((N, H, W, self.cout), dtype=torch.bfloat16, device=x.device)
        for a in range(min(d, H)):
            for b in range(min(d, W)):
                ys = hip.conv2d_fwd(x[:, a::d, b::d, :].contiguous(), self.w, self.cout, 3, 3, 1, 1, epilogue=epilogue,
                                    ep_beta=self.b, tag=self.tag, k_order=self.k_order)
                y[:, a::d, b::d, :] = ys
        return y


class HipHead(object):
    """Folded, fused inference head built from (layer2, layer3, layer4, avgpool, fc) torch modules."""

    def __init__(self, layers, fc):
        self.blocks = []
        for li, layer in layers:
            for bi, blk in enumerate(layer):
                if not isinstance(blk, Bottleneck):
                    raise hip.Sc2Error('HipHead supports torchvision Bottleneck blocks, got {}'.format(type(blk)))
                t = 'head.{}.{}'.format(li, bi)
                ds = None
                if blk.downsample is not None:
                    ds = _Conv(blk.downsample[0], blk.downsample[1], t + '.ds')
                self.blocks.append((_Conv(blk.conv1, blk.bn1, t + '.c1'), _Conv(blk.conv2, blk.bn2, t + '.c2'),
                                    _Conv(blk.conv3, blk.bn3, t + '.c3'), ds))
        self.fc = None
        if fc is not None:
            w = fc.weight.detach().float().reshape(fc.out_features, fc.in_features, 1, 1)
            cout_pad = (fc.out_features + 7) // 8 * 8
            if cout_pad != fc.out_features:
                w = torch.cat([w, torch.zeros(cout_pad - fc.out_features, fc.in_features, 1, 1, device=w.device)])
            b = torch.zeros(cout_pad, device=w.device)
            if fc.bias is not None:
                b[:fc.out_features] = fc.bias.detach().float()
            self.fc = (hip.pack_conv_weight(w), b.contiguous(), cout_pad, fc.out_features)
            # the dedicated classifier kernel (K split over the waves of a workgroup): rows padded to a multiple of 16
            self.fc_frag = None
            if fc.in_features % 128 == 0 and hip.host_policy.fc_kernel:
                n16 = (fc.out_features + 15) // 16 * 16
                w16 = torch.zeros(n16, fc.in_features, device=w.device)
                w16[:fc.out_features] = fc.weight.detach().float()
                b16 = torch.zeros(n16, device=w.device)
                if fc.bias is not None:
                    b16[:fc.out_features] = fc.bias.detach().float()
                self.fc_frag = (hip.pack_weight_fragments(w16), b16.contiguous())

    @staticmethod
    def _pair_ok(c3, c1n):
        return (c3.k == (1, 1) and c1n.k == (1, 1) and c3.stride == (1, 1) and c1n.stride == (1, 1) and c3.stream and
                c3.w2d is not None and c1n.w2d is not None and c3.w2d.shape[0] == c1n.w2d.shape[1] and
                hip.conv1x1_pair_supported(c3.w2d.shape[1], c3.cout, c1n.cout))

    def tail_spec(self):
        """(W1 [128, 256], bias1, Wds [512, 256], bias_ds) of the first block when it is layer2.0 of a ResNet-50 tail (conv1 1x1
        256 -> 128 stride 1, downsample 1x1 256 -> 512 stride 2) -- the two layers `sc2_conv2x2_win_tail_fwd` can take along
        with the last decoder conv; else None."""
        c1, _, _, ds = self.blocks[0]
        if ds is None or c1.w2d is None or ds.w2d is None:
            return None
        if tuple(c1.w2d.shape) != (128, 256) or c1.stride != (1, 1) or tuple(ds.w2d.shape) != (512, 256) or ds.stride != (2, 2):
            return None
        return c1.w2d, c1.b, ds.w2d, ds.b

    def _side_stream(self, t):
        """the side stream that belongs to the caller's current stream (one per current stream: two pipelines' back stages do not
        meet on one side stream); None while the current stream is being captured into a graph"""
        if not t.is_cuda or torch.cuda.is_current_stream_capturing():
            return None
        cur = torch.cuda.current_stream(t.device)
        pool = self.__dict__.setdefault('_side_streams', {})
        s = pool.get(cur.cuda_stream)
        if s is None:
            s = pool[cur.cuda_stream] = torch.cuda.Stream(device=t.device)
        return s

    def forward(self, x_nhwc, with_pool=True, pre=None):
        """x_nhwc: bf16 [N,H,W,C] -> logits f32 [N,classes] (or pooled / feature map if the model skips them).
        pre = (conv1 output, downsample output) of the first block when the decoder's last launch produced them."""
        h = x_nhwc
        o_next = None      # conv1 output of the coming block, when the previous block's last launch produced it
        # Round 6 A/B, default OFF: a block's downsample (layer3.0 / layer4.0: a long-K strided 1x1 layer, 0.09 - 0.11 ms at 40 - 50 %
        # of its floor rate) has no consumer until conv3, so it can run on a side stream beside conv1 -> conv2 of the same block
        # (`host_policy.head_ds_side_stream`; fork / join by events).  Measured: the two launches take each other's CUs and the
        # head gets SLOWER, 2.60 -> 2.67 ms (profiles/r06e_ab_ds_side.txt)
        side = self._side_stream(h if h is not None else pre[0]) if hip.host_policy.head_ds_side_stream else None
        for bi, (c1, c2, c3, ds) in enumerate(self.blocks):
            join = None
            if bi == 0 and pre is not None:
                o, identity = pre
            else:
                if ds is not None and side is not None:
                    cur = torch.cuda.current_stream(h.device)
                    fork = torch.cuda.Event()
                    fork.record(cur)
                    side.wait_event(fork)
                    h.record_stream(side)
                    with torch.cuda.stream(side):
                        identity = ds(h, hip.EPI_BIAS)
                        join = torch.cuda.Event()
                        join.record(side)
                    identity.record_stream(cur)
                else:
                    identity = h if ds is None else ds(h, hip.EPI_BIAS)
                o = o_next if o_next is not None else c1(h, hip.EPI_BIAS_RELU)
            o_next = None
            o = c2(o, hip.EPI_BIAS_RELU)
            if join is not None:
                torch.cuda.current_stream(h.device).wait_event(join)
            nxt = self.blocks[bi + 1] if bi + 1 < len(self.blocks) else None
            if nxt is not None and self._pair_ok(c3, nxt[0]) and hip._fits32(o.numel() // o.shape[-1] * c3.cout):
                # conv3 + residual + ReLU of this block and conv1 + ReLU of the next in one launch (conv1x1_pair.hip): the
                # block output is written once and feeds the second GEMM from LDS (layer2's block boundaries, and layer2.3 ->
                # layer3.0, whose downsample then reads the block output as any other identity path does)
                h, o_next = hip.conv1x1_pair_fwd(o, c3.packed('frag'), c3.b, identity.contiguous(), nxt[0].packed('frag'), nxt[0].b,
                                                 tag=c3.tag + '+' + nxt[0].tag)
            else:
                h = c3(o, hip.EPI_BIAS_ADD_RELU, ep_x=identity)
        if not with_pool:
            return h.permute(0, 3, 1, 2)
        if self.fc is None:                                       # [N, C] (AdaptiveAvgPool2d((1,1)) + flatten)
            return hip.avgpool_nhwc(h.contiguous(), want_f32=True)[0]
        w, b, cout_pad, n_cls = self.fc
        pooled = hip.avgpool_nhwc(h.contiguous(), want_f32=False, want_bf16=True)[1]   # f32 mean, rounded once
        if self.fc_frag is not None:
            return hip.fc_fwd(pooled, self.fc_frag[0], self.fc_frag[1], tag='head.fc')[:, :n_cls]
        pin = pooled.reshape(pooled.shape[0], 1, 1, pooled.shape[1])
        out = hip.conv2d_fwd(pin, w, cout_pad, 1, 1, 1, 0, epilogue=hip.EPI_BIAS, ep_beta=b,
                             out_format=hip.OUT_F32_NHWC, tag='head.fc')
        return out.reshape(out.shape[0], cout_pad)[:, :n_cls]


class HipResNet(object):
    """A whole torchvision-layout ResNet (`resnet.ResNet`: stem conv 7x7 + norm + ReLU, max-pool, layer1..4, avgpool, fc) in eval
    mode on the library's kernels: the classifier behind a neural INPUT codec (sc2bench/models/wrapper.py:80-135,
    `NeuralInputCompressionClassifier`, BASELINE config 3), which the reference leaves to cuDNN.  On torch ops in f32 that
    classifier went to MIOpen's `naive_conv_*` kernels and took three quarters of a step (rocprofv3 of
    `bench.py --workload fp_input`, round 5).  bf16 operands, f32 accumulation, as the Entropic-Student head."""

    def __init__(self, model):
        w = model.conv1.weight.detach().float()
        cin_pad = (w.shape[1] + 7) // 8 * 8
        if cin_pad != w.shape[1]:      # 3 input channels -> 8 (zeros): the kernels read 16-byte channel runs
            w = torch.cat([w, w.new_zeros(w.shape[0], cin_pad - w.shape[1], w.shape[2], w.shape[3])], 1)
        self.cin_pad = cin_pad
        self.stem = _Conv(ConvSpec(w, model.conv1.stride, model.conv1.padding), model.bn1, 'clf.stem')
        self.pool = (model.maxpool.kernel_size, model.maxpool.stride, model.maxpool.padding)
        self.pool_hip = model.maxpool.dilation in (1, (1, 1)) and not model.maxpool.ceil_mode and not model.maxpool.return_indices
        self.head = HipHead([(i + 1, layer) for i, layer in enumerate((model.layer1, model.layer2, model.layer3, model.layer4))], model.fc)
        self.key = self.version_key(model)

    @staticmethod
    def version_key(model):
        return tuple((t.data_ptr(), t._version) for t in list(model.parameters()) + list(model.buffers()))

    @staticmethod
    def supported(model):
        from .resnet import ResNet
        return (isinstance(model, ResNet) and not model.training and model.conv1.bias is None and model.conv1.groups == 1 and
                isinstance(model.bn1, (nn.BatchNorm2d, FrozenBatchNorm2d)) and isinstance(model.maxpool, nn.MaxPool2d) and
                all(c.dilation == (1, 1) for layer in (model.layer1, model.layer2, model.layer3, model.layer4) for b in layer
                    for c in (b.conv1, b.conv2, b.conv3)))

    def forward(self, x):
        """f32 (or bf16) NCHW image batch -> f32 logits [N, classes]"""
        x_nhwc = hip.nchw_f32_to_nhwc_bf16(x.float().contiguous(), self.cin_pad)
        h = self.stem(x_nhwc, hip.EPI_BIAS_RELU)
        k, st, pd = self.pool
        if self.pool_hip and hip.host_policy.maxpool_hip and h.shape[3] % 8 == 0:
            h = hip.maxpool_nhwc(h, k, st, pd, tag='clf.maxpool')      # (bit-identical to torch's kernel; 0.30 -> 0.13 ms at bs 256)
        else:
            h = nn.functional.max_pool2d(h.permute(0, 3, 1, 2), k, st, pd).permute(0, 2, 3, 1).contiguous()   # channels_last: a view
        return self.head.forward(h, with_pool=True)
