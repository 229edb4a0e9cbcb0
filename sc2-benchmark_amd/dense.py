"""Dense-prediction models around the bottleneck: the callers of the hot path at the shapes of BASELINE configs 4 and 5
(sc2bench/models/detection/{base,rcnn}.py, sc2bench/models/segmentation/{base,deeplabv3}.py).

What is built here, against the reference's contract (registries, constructor keywords from the YAML files, module
paths `backbone.body.bottleneck_layer` / `backbone.bottleneck_layer`, update / aux-module / analysis delegation):

* `UpdatableBackboneWithFPN` (detection/base.py:44-129): `FeatureExtractionBackbone` body + feature pyramid.  The
  pyramid (`FeaturePyramidNetwork`, `LastLevelMaxPool`) is restated on torch ops with torchvision's parameter names
  (`inner_blocks.{i}.0`, `layer_blocks.{i}.0`) -- torchvision is not installed here.
* `BaseSegmentationModel`, `deeplabv3_model` (segmentation/base.py:42-139, deeplabv3.py:44-104) with `DeepLabHead`
  (ASPP, rates 12 / 24 / 36) and `FCNHead` restated on torch ops, torchvision parameter names.
* `BaseRCNN`, `faster_rcnn_model` (detection/rcnn.py:26-226): the updatable shell.  RPN, RoI heads, anchor generator
  and the image-list transform are torchvision's `FasterRCNN` when torchvision is importable; without it they are
  `detection.FasterRCNN`, this package's restatement of the inference path (NMS and RoIAlign on csrc/detect.hip).

* `fasterrcnn_resnet50_fpn`, `deeplabv3_resnet50`: torchvision's plain models (no bottleneck) under the same registries -- the
  task models of the input-compression baselines (`wrapper.InputCompressionDetectionModel`,
  `wrapper.CodecInputCompressionSegmentationModel`).

These heads run on torch ops (MIOpen) in f32 or bf16; the bottleneck and the undilated ResNet stacks under them run on
the HIP library (`FeatureExtractionBackbone.set_compute_dtype('bf16')`).
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from .analysis import AnalyzableModule
from .backbone import FeatureExtractionBackbone, check_if_updatable
from .resnet import FrozenBatchNorm2d

DETECTION_MODEL_FUNC_DICT = dict()
SEGMENTATION_MODEL_FUNC_DICT = dict()


def register_detection_model_func(func):
    DETECTION_MODEL_FUNC_DICT[func.__name__] = func
    return func


def register_segmentation_model_func(func):
    SEGMENTATION_MODEL_FUNC_DICT[func.__name__] = func
    return func


# ------------------------------------------------------------------------------------------------ torchvision pieces
class LastLevelMaxPool(nn.Module):
    """Extra pyramid level: stride-2 subsampling of the coarsest map (torchvision.ops.feature_pyramid_network)."""

    def forward(self, results, x, names):
        names.append('pool')
        results.append(F.max_pool2d(results[-1], kernel_size=1, stride=2, padding=0))
        return results, names


class FeaturePyramidNetwork(nn.Module):
    """Top-down pyramid: 1x1 lateral convs, nearest upsampling, 3x3 output convs (Lin et al. 2017, as torchvision)."""

    def __init__(self, in_channels_list, out_channels, extra_blocks=None):
        super().__init__()
        self.inner_blocks = nn.ModuleList()
        self.layer_blocks = nn.ModuleList()
        for in_channels in in_channels_list:
            if in_channels == 0:
                raise ValueError('in_channels=0 is currently not supported')
            self.inner_blocks.append(nn.Sequential(nn.Conv2d(in_channels, out_channels, 1)))
            self.layer_blocks.append(nn.Sequential(nn.Conv2d(out_channels, out_channels, 3, padding=1)))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.extra_blocks = extra_blocks

    def forward(self, x):
        names = list(x.keys())
        feats = list(x.values())
        last_inner = self.inner_blocks[-1](feats[-1])
        results = [self.layer_blocks[-1](last_inner)]
        for idx in range(len(feats) - 2, -1, -1):
            lateral = self.inner_blocks[idx](feats[idx])
            top_down = F.interpolate(last_inner, size=lateral.shape[-2:], mode='nearest')
            last_inner = lateral + top_down
            results.insert(0, self.layer_blocks[idx](last_inner))
        if self.extra_blocks is not None:
            results, names = self.extra_blocks(results, feats, names)
        return OrderedDict(zip(names, results))


class ASPPConv(nn.Sequential):
    def __init__(self, in_channels, out_channels, dilation):
        super().__init__(nn.Conv2d(in_channels, out_channels, 3, padding=dilation, dilation=dilation, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU())


class ASPPPooling(nn.Sequential):
    def __init__(self, in_channels, out_channels):
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU())

    def forward(self, x):
        size = x.shape[-2:]
        for mod in self:
            x = mod(x)
        return F.interpolate(x, size=size, mode='bilinear', align_corners=False)


class ASPP(nn.Module):
    def __init__(self, in_channels, atrous_rates, out_channels=256):
        super().__init__()
        modules = [nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU())]
        modules += [ASPPConv(in_channels, out_channels, rate) for rate in atrous_rates]
        modules.append(ASPPPooling(in_channels, out_channels))
        self.convs = nn.ModuleList(modules)
        self.project = nn.Sequential(nn.Conv2d(len(self.convs) * out_channels, out_channels, 1, bias=False),
                                     nn.BatchNorm2d(out_channels), nn.ReLU(), nn.Dropout(0.5))

    def forward(self, x):
        return self.project(torch.cat([conv(x) for conv in self.convs], dim=1))


class DeepLabHead(nn.Sequential):
    def __init__(self, in_channels, num_classes):
        super().__init__(ASPP(in_channels, [12, 24, 36]), nn.Conv2d(256, 256, 3, padding=1, bias=False),
                         nn.BatchNorm2d(256), nn.ReLU(), nn.Conv2d(256, num_classes, 1))


class FCNHead(nn.Sequential):
    def __init__(self, in_channels, channels):
        inter = in_channels // 4
        super().__init__(nn.Conv2d(in_channels, inter, 3, padding=1, bias=False), nn.BatchNorm2d(inter), nn.ReLU(),
                         nn.Dropout(0.1), nn.Conv2d(inter, channels, 1))


class HipDenseHead(object):
    """A segmentation head (`DeepLabHead` / `FCNHead`) or a feature pyramid in eval mode on the library's kernels: every
    conv (+ BatchNorm) (+ ReLU) is ONE folded `sc2_conv2d_fwd` launch on bf16 NHWC maps, the atrous branches of the ASPP
    (sc2bench/models/segmentation/deeplabv3.py: rates 12 / 24 / 36 over the 2048-channel map) through the dilation field of the
    descriptor.  Round 5: on torch ops these layers went to MIOpen's `naive_conv_*` kernels in bf16 (rocprofv3 of
    `bench.py --workload seg513`: 90 % of the GPU time of a step) -- the reference leaves them to cuDNN, which has tuned
    kernels for them; this is that role on this hardware."""

    def __init__(self, module):
        from .head import ConvSpec, _Conv
        self._Conv, self._ConvSpec = _Conv, ConvSpec
        self.module = module
        self.key = self.version_key(module)
        self.n_out = None
        if isinstance(module, FeaturePyramidNetwork):
            self.inner = [self._plain(b[0], 'fpn.inner{}'.format(i)) for i, b in enumerate(module.inner_blocks)]
            self.layer = [self._plain(b[0], 'fpn.layer{}'.format(i)) for i, b in enumerate(module.layer_blocks)]
            self.steps = None
        else:
            self.steps = self._sequence(list(module), 'seg')

    @staticmethod
    def version_key(module):
        return tuple((t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers()))

    @staticmethod
    def supported(module):
        if isinstance(module, FeaturePyramidNetwork):
            return all(isinstance(b[0], nn.Conv2d) and b[0].groups == 1 for b in list(module.inner_blocks) + list(module.layer_blocks))
        if not isinstance(module, nn.Sequential):
            return False
        ok = (nn.Conv2d, nn.BatchNorm2d, FrozenBatchNorm2d, nn.ReLU, nn.Dropout, ASPP)
        return all(isinstance(m, ok) for m in module) and all(m.groups == 1 for m in module.modules() if isinstance(m, nn.Conv2d))

    def _plain(self, conv, tag):
        """a convolution with (or without) its own bias and no norm layer: -> (_Conv on Cout padded to a multiple of 8, Cout)"""
        cout = conv.out_channels
        cpad = (cout + 7) // 8 * 8
        w = conv.weight.detach().float()
        b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(cout, device=w.device)
        if cpad != cout:
            w = torch.cat([w, torch.zeros((cpad - cout,) + tuple(w.shape[1:]), device=w.device)])
            b = torch.cat([b, torch.zeros(cpad - cout, device=w.device)])
        c = self._Conv(self._ConvSpec(w, conv.stride, conv.padding, conv.dilation), None, tag)
        c.b = b.contiguous()
        return c, cout

    def _sequence(self, mods, tag):
        """[(kind, payload, relu)]: 'conv' (folded conv + norm), 'plain' (conv with bias), 'aspp'"""
        from . import hip
        steps, i = [], 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, ASPP):
                branches = []
                for bi, br in enumerate(m.convs):
                    if isinstance(br, ASPPPooling):
                        branches.append(('pool', self._Conv(br[1], br[2], '{}.aspp.pool'.format(tag))))
                    else:
                        branches.append(('conv', self._Conv(br[0], br[1], '{}.aspp.{}'.format(tag, bi))))
                steps.append(('aspp', (branches, self._Conv(m.project[0], m.project[1], '{}.aspp.project'.format(tag))), True))
                i += 1
            elif isinstance(m, nn.Conv2d):
                nxt = mods[i + 1] if i + 1 < len(mods) else None
                if isinstance(nxt, (nn.BatchNorm2d, FrozenBatchNorm2d)) and m.bias is None:
                    relu = i + 2 < len(mods) and isinstance(mods[i + 2], nn.ReLU)
                    steps.append(('conv', self._Conv(m, nxt, '{}.{}'.format(tag, i)), relu))
                    i += 3 if relu else 2
                else:
                    relu = isinstance(nxt, nn.ReLU)
                    steps.append(('plain', self._plain(m, '{}.{}'.format(tag, i)), relu))
                    i += 2 if relu else 1
            elif isinstance(m, (nn.Dropout, nn.ReLU)):
                i += 1
            else:
                raise hip.Sc2Error('HipDenseHead: unsupported module {}'.format(type(m).__name__))
        return steps

    def _aspp(self, x, branches, project):
        from . import hip
        N, H, W, _ = x.shape
        outs = []
        for kind, c in branches:
            if kind == 'pool':     # AdaptiveAvgPool2d(1) -> 1x1 conv + norm + ReLU -> bilinear resize of a 1 x 1 map = a broadcast
                pooled = hip.avgpool_nhwc(x, want_f32=False, want_bf16=True)[1].view(N, 1, 1, -1)
                outs.append(c(pooled, hip.EPI_BIAS_RELU).expand(N, H, W, c.cout))
            else:
                outs.append(c(x, hip.EPI_BIAS_RELU))
        return project(torch.cat(outs, dim=3), hip.EPI_BIAS_RELU)

    def __call__(self, feat):
        """feat: bf16 [N,C,H,W] (any memory format) -> bf16 logits [N,classes,H,W] (a view of NHWC memory)"""
        from . import hip
        x = feat.permute(0, 2, 3, 1).contiguous()      # a view when `feat` is channels_last (the HIP stacks' output)
        n_out = x.shape[3]
        for kind, payload, relu in self.steps:
            if kind == 'aspp':
                x = self._aspp(x, *payload)
                n_out = x.shape[3]
            elif kind == 'conv':
                x = payload(x, hip.EPI_BIAS_RELU if relu else hip.EPI_BIAS)
                n_out = payload.cout
            else:
                c, n_out = payload
                x = c(x, hip.EPI_BIAS_RELU if relu else hip.EPI_BIAS)
        return x[..., :n_out].permute(0, 3, 1, 2)

    def fpn(self, feats):
        """torchvision's FeaturePyramidNetwork.forward on bf16 maps: lateral 1x1 convs, top-down nearest upsampling + add,
        3x3 output convs; -> (results, names) in the module's order (extra blocks are applied by the caller)."""
        from . import hip
        names = list(feats.keys())
        xs = [v.permute(0, 2, 3, 1).contiguous() for v in feats.values()]
        last_inner = self.inner[-1][0](xs[-1], hip.EPI_BIAS)
        results = [self.layer[-1][0](last_inner, hip.EPI_BIAS)]
        for idx in range(len(xs) - 2, -1, -1):
            lateral = self.inner[idx][0](xs[idx], hip.EPI_BIAS)
            top_down = F.interpolate(last_inner.permute(0, 3, 1, 2), size=lateral.shape[1:3], mode='nearest').permute(0, 2, 3, 1)
            last_inner = (lateral + top_down).contiguous()
            results.insert(0, self.layer[idx][0](last_inner, hip.EPI_BIAS))
        return [r.permute(0, 3, 1, 2) for r in results], names


def _hip_dense_head(owner, module, x):
    """The cached `HipDenseHead` of `module` if this call can run on it (eval mode, bf16 parameters and bf16 features on a HIP
    device, a supported structure), else None (the torch modules run)."""
    from . import hip
    p = next(module.parameters(), None)
    if (module.training or p is None or p.dtype != torch.bfloat16 or not x.is_cuda or x.dtype != torch.bfloat16 or
            not hip.host_policy.dense_head or not HipDenseHead.supported(module)):
        return None
    cache = owner.__dict__.setdefault('_hip_dense_heads', {})
    ent = cache.get(id(module))
    if ent is None or ent.module is not module or ent.key != HipDenseHead.version_key(module):
        ent = HipDenseHead(module)
        cache[id(module)] = ent
    return ent


# ------------------------------------------------------------------------------------------------ shared behaviour
class _UpdatableDenseModel(AnalyzableModule):
    """Analysis / update calls reach the feature-extraction body that holds the bottleneck (`_body()`)."""

    def __init__(self, analyzer_configs=None):
        super().__init__(analyzer_configs)
        self.bottleneck_updated = False

    def _body(self):
        raise NotImplementedError()

    def update(self, **kwargs):
        body = self._body()
        if not check_if_updatable(body):
            raise KeyError('`backbone` {} is not updatable'.format(type(self)))
        body.update()
        self.bottleneck_updated = True

    def get_aux_module(self, **kwargs):
        return self._body().get_aux_module()

    def activate_analysis(self):
        self.activated_analysis = True
        self._body().activate_analysis()

    def deactivate_analysis(self):
        self.activated_analysis = False
        self._body().deactivate_analysis()

    def analyze(self, compressed_obj):
        if not self.activated_analysis:
            return
        for analyzer in self.analyzers:
            analyzer.analyze(compressed_obj)
        self._body().analyze(compressed_obj)

    def summarize(self):
        for analyzer in self.analyzers:
            analyzer.summarize()
        self._body().summarize()

    def clear_analysis(self):
        for analyzer in self.analyzers:
            analyzer.clear()
        self._body().clear_analysis()

    # ---- the updated eval forward in stages (pipeline.StagePipeline): the body's stages, the dense head behind its back stage.
    #      meta = (the body's meta, input height x width): the segmentation head resizes to the input
    @property
    def stage_front_takes_out(self):
        return bool(getattr(self._body(), 'stage_front_takes_out', False))

    @property
    def stage_coder_kwargs(self):
        return dict(getattr(self._body(), 'stage_coder_kwargs', {}))

    def stages_ready(self):
        body = self._body()
        return hasattr(body, 'stages_ready') and body.stages_ready()

    def stage_front(self, x, out=None):
        payload, meta = self._body().stage_front(x, out=out) if out is not None else self._body().stage_front(x)
        return payload, (meta, tuple(x.shape[-2:]))

    def stage_coder(self, payload, meta, **kwargs):
        return self._body().stage_coder(payload, meta[0], **kwargs)

    def stage_back(self, decoded, meta):
        return self._finish(self._body().stage_back(decoded, meta[0]), meta[1])

    def _finish(self, features, input_shape):
        raise NotImplementedError()


# ------------------------------------------------------------------------------------------------ detection
class UpdatableBackboneWithFPN(_UpdatableDenseModel):
    """Feature-extraction body (with the bottleneck) + FPN: the `backbone` of the R-CNN models."""

    def __init__(self, backbone, return_layer_dict, in_channels_list, out_channels, extra_blocks=None,
                 analyzer_configs=None, analyzes_after_compress=False, analyzable_layer_key=None):
        super().__init__()
        self.body = FeatureExtractionBackbone(backbone, return_layer_dict=return_layer_dict,
                                              analyzer_configs=analyzer_configs or list(),
                                              analyzes_after_compress=analyzes_after_compress,
                                              analyzable_layer_key=analyzable_layer_key)
        self.fpn = FeaturePyramidNetwork(in_channels_list=in_channels_list, out_channels=out_channels,
                                         extra_blocks=LastLevelMaxPool() if extra_blocks is None else extra_blocks)
        self.out_channels = out_channels
        self.analyzable_layer_key = analyzable_layer_key

    def _body(self):
        return self.body

    def _finish(self, feats, input_shape=None):
        ref_dtype = self.fpn.inner_blocks[0][0].weight.dtype
        feats = OrderedDict((k, v.to(ref_dtype)) for k, v in feats.items())
        hd = _hip_dense_head(self, self.fpn, next(iter(feats.values())))
        if hd is not None:       # the pyramid's 1x1 / 3x3 convs on the library's kernels (bf16 eval)
            results, names = hd.fpn(feats)
            if self.fpn.extra_blocks is not None:
                results, names = self.fpn.extra_blocks(results, list(feats.values()), names)
            return OrderedDict(zip(names, results))
        return self.fpn(feats)

    def forward(self, x):
        return self._finish(self.body(x))

    def check_if_updatable(self):
        return self.body.check_if_updatable()


def backbone_with_fpn(backbone, extra_blocks=None, return_layer_dict=None, in_channels_list=None, in_channels_stage2=None,
                      out_channels=256, returned_layers=None, analysis_config=None, analyzable_layer_key=None):
    """The backbone half of `create_faster_rcnn_fpn` (detection/rcnn.py:113-165): defaults for the returned layers and
    the pyramid's channel counts derived from `backbone.inplanes`."""
    analysis_config = analysis_config or dict()
    if returned_layers is None:
        returned_layers = [1, 2, 3, 4]
    if return_layer_dict is None:
        return_layer_dict = {'layer{}'.format(k): str(v) for v, k in enumerate(returned_layers)}
    if in_channels_stage2 is None:
        in_channels_stage2 = backbone.inplanes // 8
    if in_channels_list is None:
        in_channels_list = [in_channels_stage2 * 2 ** (i - 1) for i in returned_layers]
    return UpdatableBackboneWithFPN(backbone, return_layer_dict, in_channels_list, out_channels, extra_blocks=extra_blocks,
                                    analyzable_layer_key=analyzable_layer_key, **analysis_config)


class BaseRCNN(_UpdatableDenseModel):
    """Updatable generalized R-CNN: transform -> backbone (body + FPN) -> RPN -> RoI heads -> postprocess, with the
    pieces handed in (torchvision's, or anything with the same call signatures)."""

    def __init__(self, rcnn_model, analysis_config=None):
        analysis_config = analysis_config or dict()
        super().__init__(analysis_config.get('analyzer_configs', list()))
        self.transform = rcnn_model.transform
        self.backbone = rcnn_model.backbone
        self.rpn = rcnn_model.rpn
        self.roi_heads = rcnn_model.roi_heads

    def _body(self):
        return self.backbone.body

    def forward(self, images, targets=None):
        if self.training and targets is None:
            raise ValueError('targets should not be None in training mode')
        from .detection import original_sizes
        original_image_sizes = original_sizes(images)      # (a planned batch states them: transforms.DeferredDetBatch.sizes)
        images, targets = self.transform(images, targets)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([('0', features)])
        proposals, proposal_losses = self.rpn(images, features, targets)
        detections, detector_losses = self.roi_heads(features, proposals, images.image_sizes, targets)
        detections = self.transform.postprocess(detections, images.image_sizes, original_image_sizes)
        if self.training:
            losses = dict(detector_losses)
            losses.update(proposal_losses)
            return losses
        return detections


@register_detection_model_func
def faster_rcnn_model(backbone_config, pretrained=True, pretrained_backbone_name=None, progress=True,
                      backbone_fpn_kwargs=None, num_classes=91, analysis_config=None, start_ckpt_file_path=None, **kwargs):
    """Faster R-CNN with a splittable backbone + FPN (detection/rcnn.py:183-226).  The backbone is built with
    FrozenBatchNorm2d as the reference does; RPN / RoI heads / transform come from torchvision's FasterRCNN where it is
    importable, else from `detection.FasterRCNN`."""
    from .wrapper import load_classification_model
    backbone_fpn_kwargs = dict(backbone_fpn_kwargs or {})
    backbone_config = dict(backbone_config, kwargs=dict(backbone_config.get('kwargs') or {}, norm_layer='FrozenBatchNorm2d'))
    backbone = load_classification_model(backbone_config, torch.device('cpu'), strict=False)
    bfpn = backbone_with_fpn(backbone, **backbone_fpn_kwargs)
    try:
        from torchvision.models.detection.faster_rcnn import FasterRCNN
    except ImportError:       # the package's own restatement of the inference path, NMS and RoIAlign on the library's kernels
        from .detection import FasterRCNN
    model = BaseRCNN(FasterRCNN(bfpn, num_classes, **kwargs), analysis_config=analysis_config)
    if pretrained and pretrained_backbone_name:
        import logging
        logging.getLogger(__name__).warning('faster_rcnn_model: pretrained COCO weights are a download upstream; pass '
                                            'start_ckpt_file_path to load a local checkpoint')
    if start_ckpt_file_path is not None:
        from .ckpt import load_ckpt
        load_ckpt(start_ckpt_file_path, model=model, strict=False)
    return model


def _no_pretrained(name, start_ckpt_file_path):
    if start_ckpt_file_path is None:
        import logging
        logging.getLogger(__name__).warning('{}: pretrained weights are a download upstream; pass start_ckpt_file_path to load a '
                                            'local checkpoint'.format(name))


@register_detection_model_func
def fasterrcnn_resnet50_fpn(pretrained=False, progress=True, num_classes=91, start_ckpt_file_path=None, **kwargs):
    """torchvision's `fasterrcnn_resnet50_fpn` (the detector of the input-compression baselines): a plain ResNet-50 with
    FrozenBatchNorm2d under the feature pyramid, `FasterRCNN` from torchvision where it is importable, else `detection.FasterRCNN`
    (inference only).  State-dict names are torchvision's (`backbone.body.*`, `backbone.fpn.*`, `rpn.*`, `roi_heads.*`)."""
    from .resnet import resnet50
    bfpn = backbone_with_fpn(resnet50(norm_layer=FrozenBatchNorm2d))
    try:
        from torchvision.models.detection.faster_rcnn import FasterRCNN
    except ImportError:
        from .detection import FasterRCNN
    model = FasterRCNN(bfpn, num_classes, **kwargs)
    if pretrained:
        _no_pretrained('fasterrcnn_resnet50_fpn', start_ckpt_file_path)
    if start_ckpt_file_path is not None:
        from .ckpt import load_ckpt
        load_ckpt(start_ckpt_file_path, model=model, strict=False)
    return model


# ------------------------------------------------------------------------------------------------ segmentation
class BaseSegmentationModel(_UpdatableDenseModel):
    """backbone features -> classifier (-> aux classifier), bilinearly resized to the input (segmentation/base.py:42-81)."""

    def __init__(self, backbone, classifier, aux_classifier=None, analysis_config=None):
        analysis_config = analysis_config or dict()
        super().__init__(analysis_config.get('analyzer_configs', list()))
        self.backbone = backbone
        self.classifier = classifier
        self.aux_classifier = aux_classifier
        self.defer_resize = False     # True (training mode only): forward returns `ResizedLogits`, the criterion resizes inside its loss kernel

    def _body(self):
        return self.backbone

    def _logits(self, head, feat):
        """the head's low-resolution logits [N,classes,h,w]: a permuted view of NHWC memory from the library's kernels, NCHW from torch's"""
        w = next(head.parameters())
        feat = feat.to(w.dtype)
        hd = _hip_dense_head(self, head, feat)
        return hd(feat) if hd is not None else head(feat)

    def _head(self, head, feat, size):
        logits = ResizedLogits(self._logits(head, feat), size)
        if self.defer_resize and self.training:
            return logits
        return logits.resized()

    def _finish(self, features, input_shape):
        result = OrderedDict()
        result['out'] = self._head(self.classifier, features['out'], input_shape)
        if self.aux_classifier is not None:
            result['aux'] = self._head(self.aux_classifier, features['aux'], input_shape)
        return result

    def forward(self, x):
        return self._finish(self.backbone(x), x.shape[-2:])

    def predict(self, x, targets=None, mat=None):
        """The evaluation tail of the reference (`model(x)['out'].argmax(1)` into `SegEvaluator.update`) without the resized
        logits: backbone -> classifier -> `seg_labels` on the low-resolution map.  -> int64 labels [N,H,W] of the input's size;
        with `targets` (int64 [N,H,W]) and `mat` (int64 [classes,classes]) the confusion counts are ADDED to `mat`.  The aux head
        does not run.  `forward` is what it was: it still returns the resized logits."""
        features = self.backbone(x)
        return seg_labels(self._logits(self.classifier, features['out']), x.shape[-2:], targets, mat)


def create_deeplabv3(backbone, num_input_channels=2048, uses_aux=False, num_aux_channels=1024, num_classes=21):
    aux_classifier = FCNHead(num_aux_channels, num_classes) if uses_aux else None
    return BaseSegmentationModel(backbone, DeepLabHead(num_input_channels, num_classes), aux_classifier)


@register_segmentation_model_func
def deeplabv3_model(backbone_config, pretrained=True, pretrained_backbone_name=None, progress=True,
                    num_input_channels=2048, uses_aux=False, num_aux_channels=1024, return_layer_dict=None,
                    num_classes=21, analysis_config=None, analyzable_layer_key=None, start_ckpt_file_path=None, **kwargs):
    """DeepLabv3 on a splittable backbone (segmentation/deeplabv3.py:44-104)."""
    from .wrapper import load_classification_model
    analysis_config = analysis_config or dict()
    if return_layer_dict is None:
        return_layer_dict = {'layer4': 'out'}
        if uses_aux:
            return_layer_dict['layer3'] = 'aux'
    backbone = load_classification_model(backbone_config, torch.device('cpu'), strict=False)
    body = FeatureExtractionBackbone(backbone, return_layer_dict, analysis_config.get('analyzer_configs', list()),
                                     analysis_config.get('analyzes_after_compress', False),
                                     analyzable_layer_key=analyzable_layer_key)
    model = create_deeplabv3(body, num_input_channels=num_input_channels, uses_aux=uses_aux,
                             num_aux_channels=num_aux_channels, num_classes=num_classes)
    if pretrained and pretrained_backbone_name:
        import logging
        logging.getLogger(__name__).warning('deeplabv3_model: pretrained COCO weights are a download upstream; pass '
                                            'start_ckpt_file_path to load a local checkpoint')
    if start_ckpt_file_path is not None:
        from .ckpt import load_ckpt
        load_ckpt(start_ckpt_file_path, model=model, strict=False)
    return model


@register_segmentation_model_func
def deeplabv3_resnet50(pretrained=False, progress=True, num_classes=21, aux_loss=None, start_ckpt_file_path=None, **kwargs):
    """torchvision's `deeplabv3_resnet50` (the segmentation model of the input-compression baselines): a plain ResNet-50 with
    dilated layer3 / layer4, `DeepLabHead`, and the `FCNHead` aux classifier with `aux_loss`.  State-dict names are torchvision's
    (`backbone.*`, `classifier.*`, `aux_classifier.*`)."""
    from .resnet import resnet50
    backbone = resnet50(replace_stride_with_dilation=[False, True, True])
    return_layer_dict = {'layer4': 'out'}
    if aux_loss:
        return_layer_dict['layer3'] = 'aux'
    body = FeatureExtractionBackbone(backbone, return_layer_dict, list())
    model = create_deeplabv3(body, uses_aux=bool(aux_loss), num_classes=num_classes)
    if pretrained:
        _no_pretrained('deeplabv3_resnet50', start_ckpt_file_path)
    if start_ckpt_file_path is not None:
        from .ckpt import load_ckpt
        load_ckpt(start_ckpt_file_path, model=model, strict=False)
    return model


# ------------------------------------------------------------------------------------------------ evaluation state
def _count_pairs(mat, target, prediction):
    """SegEvaluator.update's arithmetic on flat tensors: mat[t, p] += 1 where 0 <= t < classes."""
    n = mat.shape[0]
    keep = (target >= 0) & (target < n)
    inds = n * target[keep].to(torch.int64) + prediction[keep]
    mat += torch.bincount(inds, minlength=n ** 2).reshape(n, n)


class ResizedLogits(object):
    """Low-resolution logits [N,C,h,w] and the size they are to be resized to: what `BaseSegmentationModel.forward` returns per head
    with `defer_resize` in training mode, for a criterion that takes the resize into its own kernel (`seg_cross_entropy`)."""

    def __init__(self, logits, size):
        self.logits = logits
        self.size = (int(size[0]), int(size[1]))

    def resized(self):
        return F.interpolate(self.logits, size=self.size, mode='bilinear', align_corners=False)


class _SegCrossEntropyFn(torch.autograd.Function):
    """sc2_seg_ce_forward / sc2_seg_ce_backward; the loss leaves as an f32 device scalar ('mean', 'sum') or f32 [N,H,W] ('none')"""

    @staticmethod
    def forward(ctx, logits, size, targets, ignore_index, reduction):
        from . import hip
        res = hip.seg_ce_forward(logits, size, targets, ignore_index, want_pixel_loss=reduction == hip.SEG_CE_NONE)
        ctx.save_for_backward(logits, targets, res.lse, res.sums)
        ctx.size, ctx.ignore_index, ctx.reduction = size, ignore_index, reduction
        ctx.mark_non_differentiable(res.sums)
        if reduction == hip.SEG_CE_NONE:
            return res.pixel_loss, res.sums
        if reduction == hip.SEG_CE_SUM:
            return res.sums[0].float(), res.sums
        return (res.sums[0] / res.sums.view(torch.int64)[1]).float(), res.sums      # 0 / 0 = NaN, as torch

    @staticmethod
    def backward(ctx, grad_out, _grad_sums):
        from . import hip
        logits, targets, lse, sums = ctx.saved_tensors
        dx = hip.seg_ce_backward(logits, ctx.size, targets, lse, sums, grad_out.float().contiguous(), ctx.ignore_index, ctx.reduction)
        return dx, None, None, None, None


def seg_cross_entropy(logits, size, targets, ignore_index=255, reduction='mean', strict=False, weight=None, label_smoothing=0.0):
    """`F.cross_entropy(F.interpolate(logits, size, mode='bilinear', align_corners=False), targets, ignore_index=.., reduction=..)` from
    the LOW-resolution logits [N,C,h,w].  Device tensors of up to 64 classes (f32 / bf16, no class weights, no label smoothing, with
    `host_policy.seg_loss_hip` on) go to `sc2_seg_ce_forward` and, through autograd, `sc2_seg_ce_backward`: f32 arithmetic on the
    unrounded logits, neither the resized logits nor their gradient are formed, the loss is an f32 device scalar and nothing is read
    back.  Anything else takes the two torch ops.  A target outside 0..C-1 that is not `ignore_index` is skipped and counted by the
    kernels (torch asserts on the device); `strict=True` reads the count back and raises ValueError."""
    from . import hip
    size = (int(size[0]), int(size[1]))
    code = {'mean': hip.SEG_CE_MEAN, 'sum': hip.SEG_CE_SUM, 'none': hip.SEG_CE_NONE}.get(reduction)
    if (logits.is_cuda and targets.is_cuda and hip.host_policy.seg_loss_hip and code is not None and weight is None and not label_smoothing and
            logits.dim() == 4 and logits.shape[1] <= hip.SEG_MAX_CLASSES and logits.dtype in (torch.float32, torch.bfloat16)):
        loss, sums = _SegCrossEntropyFn.apply(logits, size, targets.to(torch.int64).contiguous(), int(ignore_index), code)
        if strict:
            bad = int(sums.view(torch.int64)[2])
            if bad:
                raise ValueError('seg_cross_entropy: {} targets outside 0..{} that are not ignore_index={}'.format(
                    bad, logits.shape[1] - 1, ignore_index))
        return loss
    resized = F.interpolate(logits, size=size, mode='bilinear', align_corners=False)
    return F.cross_entropy(resized, targets, weight=weight, ignore_index=ignore_index, reduction=reduction, label_smoothing=label_smoothing)


def seg_labels(logits, size, targets=None, mat=None, want_labels=True):
    """Labels of low-resolution logits [N,C,h,w] at `size` = (H, W), and (with `targets` int64 [N,H,W] and `mat` int64 [C,C]) their
    confusion counts added to `mat`.  Device tensors of up to 64 classes go to ONE launch of `sc2_seg_predict`: bilinear
    weights from integers, f32 arithmetic on the unrounded logits, no resized tensor.  CPU tensors, more classes and
    `host_policy.seg_predict_hip = False` take the torch-op restatement: interpolate in f32, argmax, bincount.
    -> int64 labels [N,H,W] (None with want_labels=False on the kernel path: nothing is stored)."""
    from . import hip
    size = (int(size[0]), int(size[1]))
    if (logits.is_cuda and hip.host_policy.seg_predict_hip and logits.shape[1] <= hip.SEG_MAX_CLASSES and
            logits.dtype in (torch.float32, torch.bfloat16)):
        if targets is not None and mat is not None:
            return hip.seg_predict(logits, size, targets.to(torch.int64).contiguous(), mat, want_labels=want_labels)
        return hip.seg_predict(logits, size)
    labels = F.interpolate(logits.float(), size=size, mode='bilinear', align_corners=False).argmax(1)
    if targets is not None and mat is not None:
        _count_pairs(mat, targets.flatten(), labels.flatten())
    return labels


class SegEvaluator(object):
    """Confusion matrix of a segmentation run and its cross-rank reduction (script/task/utils/eval.py:4-46: one int64
    [classes, classes] all-reduce -- the C4 collective of SURVEY.md 2.3)."""

    def __init__(self, num_classes):
        self.num_classes = num_classes
        self.mat = None

    def update(self, target, prediction):
        n = self.num_classes
        if self.mat is None:
            self.mat = torch.zeros((n, n), dtype=torch.int64, device=target.device)
        with torch.no_grad():
            keep = (target >= 0) & (target < n)
            inds = n * target[keep].to(torch.int64) + prediction[keep]
            self.mat += torch.bincount(inds, minlength=n ** 2).reshape(n, n)

    def update_logits(self, targets, logits):
        """`update(targets.flatten(), interpolate(logits, targets' size).argmax(1).flatten())` from the LOW-resolution logits
        [N,classes,h,w]: on a HIP device one launch that adds into the matrix (`seg_labels`), no resized tensor, no labels."""
        n = self.num_classes
        if logits.shape[1] != n:
            raise ValueError('update_logits: {} logit planes for {} classes'.format(logits.shape[1], n))
        if self.mat is None:
            self.mat = torch.zeros((n, n), dtype=torch.int64, device=targets.device)
        with torch.no_grad():
            seg_labels(logits, targets.shape[-2:], targets, self.mat, want_labels=False)

    def reset(self):
        if self.mat is not None:
            self.mat.zero_()

    def compute(self):
        h = self.mat.float()
        acc_global = torch.diag(h).sum() / h.sum() * 100.0
        acc = torch.diag(h) / h.sum(1) * 100.0
        iu = torch.diag(h) / (h.sum(1) + h.sum(0) - torch.diag(h)) * 100.0
        return acc_global, acc, iu

    def reduce_from_all_processes(self):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        dist.barrier()
        dist.all_reduce(self.mat)

    def __str__(self):
        acc_global, acc, iu = self.compute()
        return 'mean IoU: {:.1f}, IoU: {}, Global pixelwise acc: {:.1f}, Average row correct: {}'.format(
            iu.mean().item(), ['{:.1f}'.format(i) for i in iu.tolist()], acc_global.item(), ['{:.1f}'.format(i) for i in acc.tolist()])
