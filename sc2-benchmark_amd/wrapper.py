"""Model wrappers of the reference's baselines (sc2bench/models/wrapper.py), built against the same contract:
registry `WRAPPER_CLASS_DICT`, constructor keywords as the YAML files pass them, `forward` semantics, analyzers.

* `NeuralInputCompressionClassifier` (wrapper.py:80-135): pre_transform -> compression_model.compress -> analyze the
  compressed object -> decompress (`x_hat`) -> post_transform -> classifier.  BASELINE config 3 drives the HIP-backed
  `compression.FactorizedPrior` through it.
* `CodecFeatureCompressionClassifier` (wrapper.py:138-193): classifier split into encoder / decoder / classifier by
  `sequential` module lists; each sample's feature map goes through a codec transform (config 1: `PILTensorModule`).
* `CodecInputCompressionClassifier` (wrapper.py:28-77), `EntropicClassifier` (:196-265), `SplitClassifier` (:268-322).
* `InputCompressionDetectionModel` (models/detection/wrapper.py:11-95) and `CodecInputCompressionSegmentationModel`
  (models/segmentation/wrapper.py:11-51): the codec input-compression baselines of the two dense tasks, with their
  `get_wrapped_*_model` builders.

Reference behaviour kept on purpose: per-sample results are joined with `torch.hstack`, i.e. along dim 1 -- the
reference evaluates these baselines at test batch size 1 (README.md:100-108), where that equals a batch of one.
"""
from collections import OrderedDict

import torch
from torch import nn

from .analysis import AnalyzableModule
from .backbone import UpdatableBackbone
from .layer import EntropyBottleneckLayer
from .training import redesign_model
from .transforms import Compose, Normalize, PILImageModule, ToTensor, _is_pil

WRAPPER_CLASS_DICT = dict()


def register_wrapper_class(cls):
    WRAPPER_CLASS_DICT[cls.__name__] = cls
    return cls


def _section(model, config):
    """`{sequential: [...]}` -> the named children of `model` in a row; `{ignored: True}` -> identity."""
    config = config or dict()
    if config.get('ignored', False):
        return nn.Identity()
    return redesign_model(model, config.get('sequential'))


def _analyzer_configs(analysis_config):
    return (analysis_config or dict()).get('analyzer_configs', list())


class _PerSampleCodec(object):
    """codec -> analyze(file size) -> post_transform for every sample of a batch, joined as the reference joins them.  Three forms
    with one result: the loop; a 4-D tensor through `PILTensorModule.forward_batch`; a list of PIL images through
    `PILImageModule.forward_batch`."""

    def _batch_codec(self):
        """The codec when it takes a whole batch (`forward_batch` of transforms.PILTensorModule or PILImageModule, alone or as the one
        transform of a `Compose`) and reports sizes, else None."""
        codec = self.codec_encoder_decoder
        if isinstance(codec, Compose) and len(codec.transforms) == 1:
            codec = codec.transforms[0]
        return codec if hasattr(codec, 'forward_batch') and getattr(codec, 'returns_file_size', False) else None

    def _image_batch_codec(self, samples):
        """The codec when `samples` is a list of PIL images, the codec a size-reporting `transforms.PILImageModule` (alone or as the
        one transform of a `Compose`) and the post_transform one that takes the decoded pixels as a uint8 batch tensor: its
        `forward_batch` takes the whole list.  Else None: any other post_transform (a `Resize` first, a callable of the caller's)
        expects the reopened PIL image of the loop, so the decision is made before anything is launched."""
        if not isinstance(samples, (list, tuple)) or len(samples) == 0 or not all(_is_pil(sample) for sample in samples):
            return None
        if not self._post_transform_takes_batches():
            return None
        codec = self._batch_codec()
        return codec if isinstance(codec, PILImageModule) else None

    def _post_transform_takes_batches(self):
        """None, or a `Compose` of exactly `ToTensor` followed by at most one `Normalize`: element-wise on uint8 pixels, so one call on
        the decoded batch [B,C,H,W] gives what the calls on its samples give."""
        post = self.post_transform
        if post is None:
            return True
        if not isinstance(post, Compose) or not 1 <= len(post.transforms) <= 2 or type(post.transforms[0]) is not ToTensor:
            return False
        return len(post.transforms) == 1 or type(post.transforms[1]) is Normalize

    def _through_image_batch(self, codec, samples):
        decoded, sizes = codec.forward_batch(list(samples), self.device)
        if isinstance(decoded, torch.Tensor):      # the kernel path: uint8 [B,C,H,W] on the device
            if not self.training:
                for file_size in sizes:
                    self.analyze(file_size)
            batch = decoded if self.post_transform is None else self.post_transform(decoded)
            # the loop joins its [1,C,H,W] samples with torch.hstack, i.e. along dim 1: [1, B*C, H, W]
            return batch.reshape(1, -1, batch.shape[-2], batch.shape[-1]).to(self.device)
        outputs = []                               # the codec's host path: the reopened PIL images, as in the loop
        for sample, file_size in zip(decoded, sizes):
            if not self.training:
                self.analyze(file_size)
            if self.post_transform is not None:
                sample = self.post_transform(sample)
            outputs.append(sample.unsqueeze(0))
        return torch.hstack(outputs).to(self.device)

    def _through_codec(self, samples):
        codec = self._image_batch_codec(samples)
        if codec is not None:
            return self._through_image_batch(codec, samples)
        outputs = []
        codec = self._batch_codec() if isinstance(samples, torch.Tensor) and samples.dim() == 4 else None
        if codec is not None and not isinstance(codec, PILImageModule):
            features, sizes = codec.forward_batch(samples)
            for sample, file_size in zip(features, sizes):
                if not self.training:
                    self.analyze(file_size)
                if self.post_transform is not None:
                    sample = self.post_transform(sample)
                outputs.append(sample.unsqueeze(0))
            return torch.hstack(outputs).to(self.device)
        for sample in samples:
            if self.codec_encoder_decoder is not None:
                sample, file_size = self.codec_encoder_decoder(sample)
                if not self.training:
                    self.analyze(file_size)
            if self.post_transform is not None:
                sample = self.post_transform(sample)
            outputs.append(sample.unsqueeze(0))
        return torch.hstack(outputs).to(self.device)


@register_wrapper_class
class CodecInputCompressionClassifier(AnalyzableModule, _PerSampleCodec):
    """Codec (JPEG / WebP / BPG ...) on the input image, then a classifier.  `x`: list of PIL images."""

    def __init__(self, classification_model, device, codec_encoder_decoder=None, post_transform=None,
                 analysis_config=None, **kwargs):
        super().__init__(_analyzer_configs(analysis_config))
        self.codec_encoder_decoder = codec_encoder_decoder
        self.device = device
        self.classification_model = classification_model
        self.post_transform = post_transform

    def forward(self, x):
        return self.classification_model(self._through_codec(x))


@register_wrapper_class
class CodecInputCompressionSegmentationModel(AnalyzableModule, _PerSampleCodec):
    """Codec on the input image, then a segmentation model (sc2bench/models/segmentation/wrapper.py:11-51).  `x`: list of PIL
    images; equal-size images with a `ToTensor` (+ `Normalize`) post-transform take the device codec as the classifier's do."""

    def __init__(self, segmentation_model, device, codec_encoder_decoder=None, post_transform=None, analysis_config=None, **kwargs):
        super().__init__(_analyzer_configs(analysis_config))
        self.codec_encoder_decoder = codec_encoder_decoder
        self.device = device
        self.segmentation_model = segmentation_model
        self.post_transform = post_transform

    def forward(self, x):
        return self.segmentation_model(self._through_codec(x))


def _check_if_analyzable(module):
    return isinstance(module, AnalyzableModule)


@register_wrapper_class
class InputCompressionDetectionModel(AnalyzableModule):
    """Codec or compression model on the RESIZED input image, then a detection model (sc2bench/models/detection/wrapper.py:11-95):
    the detector's `transform` is replaced by `detection.RCNNTransformWithCompression`, which holds the analyzers; the five analysis
    calls are passed on to it."""

    def __init__(self, detection_model, device, codec_encoder_decoder=None, compression_model=None, uses_cpu4compression_model=False,
                 pre_transform=None, post_transform=None, analysis_config=None, adaptive_pad_kwargs=None, **kwargs):
        from .detection import RCNNTransformWithCompression
        analysis_config = analysis_config or dict()
        super().__init__()
        detection_model.transform = RCNNTransformWithCompression(
            detection_model.transform, device, codec_encoder_decoder, _analyzer_configs(analysis_config),
            analyzes_after_compress=analysis_config.get('analyzes_after_compress', False), compression_model=compression_model,
            uses_cpu4compression_model=uses_cpu4compression_model, pre_transform=pre_transform, post_transform=post_transform,
            adaptive_pad_kwargs=adaptive_pad_kwargs)
        self.device = device
        self.uses_cpu4compression_model = uses_cpu4compression_model
        self.detection_model = detection_model

    def use_cpu4compression(self):
        transform = self.detection_model.transform
        if self.uses_cpu4compression_model and transform.compression_model is not None:
            transform.compression_model = transform.compression_model.cpu()

    def forward(self, x):
        return self.detection_model(x)

    def activate_analysis(self):
        self.activated_analysis = True
        if _check_if_analyzable(self.detection_model.transform):
            self.detection_model.transform.activate_analysis()

    def deactivate_analysis(self):
        self.activated_analysis = False
        if _check_if_analyzable(self.detection_model.transform):
            self.detection_model.transform.deactivate_analysis()

    def analyze(self, compressed_obj):
        if not self.activated_analysis:
            return
        for analyzer in self.analyzers:
            analyzer.analyze(compressed_obj)
        if _check_if_analyzable(self.detection_model.transform):
            self.detection_model.transform.analyze(compressed_obj)

    def summarize(self):
        for analyzer in self.analyzers:
            analyzer.summarize()
        if _check_if_analyzable(self.detection_model.transform):
            self.detection_model.transform.summarize()

    def clear_analysis(self):
        for analyzer in self.analyzers:
            analyzer.clear()
        if _check_if_analyzable(self.detection_model.transform):
            self.detection_model.transform.clear_analysis()


@register_wrapper_class
class NeuralInputCompressionClassifier(AnalyzableModule):
    """Learned image codec on the input, then a classifier."""

    def __init__(self, classification_model, pre_transform=None, compression_model=None,
                 uses_cpu4compression_model=False, post_transform=None, analysis_config=None, **kwargs):
        analysis_config = analysis_config or dict()
        super().__init__(_analyzer_configs(analysis_config))
        self.analyzes_after_pre_transform = analysis_config.get('analyzes_after_pre_transform', False)
        self.analyzes_after_compress = analysis_config.get('analyzes_after_compress', False)
        self.pre_transform = pre_transform
        self.compression_model = compression_model
        self.uses_cpu4compression_model = uses_cpu4compression_model
        self.classification_model = classification_model
        self.post_transform = post_transform

    def use_cpu4compression(self):
        """The reference can park the codec on the CPU (wrapper.py:113-119); the HIP-backed codec has no CPU path, so a
        model that asks for it is told, not silently moved."""
        if self.uses_cpu4compression_model and self.compression_model is not None:
            from . import hip
            raise hip.Sc2Error('uses_cpu4compression_model: the compression model of this build runs on a HIP device only')

    # ---- the same forward in stages (pipeline.StagePipeline): the codec's serial range coder on its own HIP stream
    stage_front_takes_out = False
    stage_coder_kwargs = {'dequantized': True}

    def stages_ready(self):
        cm = self.compression_model
        return (cm is not None and hasattr(cm, 'stage_front') and not self.training and next(cm.parameters()).is_cuda and
                cm.entropy_bottleneck._quantized_cdf.numel() > 0)

    def stage_front(self, x, out=None):
        if self.pre_transform is not None:
            x = self.pre_transform(x)
        return self.compression_model.stage_front(x)

    def stage_coder(self, payload, meta, **kwargs):
        return self.compression_model.stage_coder(payload, meta, **kwargs)

    def stage_back(self, decoded, meta):
        x = self.compression_model.stage_back(decoded, meta)
        if self.post_transform is not None:
            x = self.post_transform(x)
        return self._classify(x)

    def set_compute_dtype(self, dtype):
        """'f32' (the reference's dtype; default): the classifier's own torch modules.  'bf16': a torchvision-layout ResNet
        classifier in eval mode runs on the library's fused conv + norm kernels (head.HipResNet), as the Entropic-Student
        model's head does; any other classifier keeps its modules."""
        assert dtype in ('f32', 'bf16')
        self.compute_dtype = dtype
        return self

    def _classify(self, x):
        clf = self.classification_model
        if getattr(self, 'compute_dtype', 'f32') == 'bf16' and x.is_cuda and not self.training:
            from .head import HipResNet
            if HipResNet.supported(clf):
                ent = self.__dict__.get('_hip_clf')
                if ent is None or ent.key != HipResNet.version_key(clf):
                    ent = HipResNet(clf)
                    self.__dict__['_hip_clf'] = ent
                return ent.forward(x)
        return clf(x)

    def forward(self, x):
        if self.pre_transform is not None:
            x = self.pre_transform(x)
            if self.analyzes_after_pre_transform and not self.training:
                self.analyze(x)
        if self.compression_model is not None:
            compressed_obj = self.compression_model.compress(x)
            if self.analyzes_after_compress and not self.training:
                self.analyze(compressed_obj)
            x = self.compression_model.decompress(**compressed_obj)
            if isinstance(x, dict):
                x = x['x_hat']
        if self.post_transform is not None:
            x = self.post_transform(x)
        return self._classify(x)


@register_wrapper_class
class CodecFeatureCompressionClassifier(AnalyzableModule, _PerSampleCodec):
    """Codec on an intermediate feature map of the classifier (the jpeg-resnet50 feature-compression baseline)."""

    def __init__(self, classification_model, device, encoder_config=None, codec_encoder_decoder=None,
                 decoder_config=None, classifier_config=None, post_transform=None, analysis_config=None, **kwargs):
        super().__init__(_analyzer_configs(analysis_config))
        self.codec_encoder_decoder = codec_encoder_decoder
        self.device = device
        self.encoder = _section(classification_model, encoder_config)
        self.decoder = _section(classification_model, decoder_config)
        self.classifier = _section(classification_model, classifier_config)
        self.post_transform = post_transform

    def forward(self, x):
        x = self._through_codec(self.encoder(x))
        x = self.decoder(x)
        return self.classifier(torch.flatten(x, 1))


class _SplitBase(UpdatableBackbone):
    def __init__(self, classification_model, encoder_config, decoder_config, classifier_config, analysis_config):
        analysis_config = analysis_config or dict()
        super().__init__(_analyzer_configs(analysis_config))
        self.analyzes_after_compress = analysis_config.get('analyzes_after_compress', False)
        self.encoder = _section(classification_model, encoder_config)
        self.decoder = _section(classification_model, decoder_config)
        self.classifier = _section(classification_model, classifier_config)

    def _tail(self, x):
        x = self.decoder(x)
        return self.classifier(torch.flatten(x, 1))


@register_wrapper_class
class EntropicClassifier(_SplitBase):
    """An `EntropyBottleneckLayer` between two halves of a classifier."""

    def __init__(self, classification_model, encoder_config, compression_model_kwargs, decoder_config,
                 classifier_config, analysis_config=None, **kwargs):
        super().__init__(classification_model, encoder_config, decoder_config, classifier_config, analysis_config)
        self.entropy_bottleneck = EntropyBottleneckLayer(**compression_model_kwargs)

    def forward(self, x):
        x = self.encoder(x)
        if self.bottleneck_updated and not self.training:
            x = self.entropy_bottleneck.compress(x)
            if self.analyzes_after_compress:
                self.analyze(x)
            x = self.entropy_bottleneck.decompress(**x)
        else:
            x, _ = self.entropy_bottleneck(x)
        return self._tail(x)

    def update(self):
        self.entropy_bottleneck.update()
        self.bottleneck_updated = True

    def load_state_dict(self, state_dict, **kwargs):
        own = OrderedDict((k[len('entropy_bottleneck.'):], state_dict.pop(k)) for k in list(state_dict.keys())
                          if k.startswith('entropy_bottleneck.'))
        super().load_state_dict(state_dict, strict=False)
        self.entropy_bottleneck.load_state_dict(own)

    def get_aux_module(self, **kwargs):
        return self.entropy_bottleneck


@register_wrapper_class
class SplitClassifier(_SplitBase):
    """A classifier split in two with an optional (de)compressor transform pair at the cut."""

    def __init__(self, classification_model, encoder_config, decoder_config, classifier_config,
                 compressor_transform=None, decompressor_transform=None, analysis_config=None, **kwargs):
        super().__init__(classification_model, encoder_config, decoder_config, classifier_config, analysis_config)
        self.compressor = compressor_transform
        self.decompressor = decompressor_transform

    def forward(self, x):
        x = self.encoder(x)
        if self.bottleneck_updated and not self.training:
            x = self.compressor(x)
            if self.analyzes_after_compress:
                self.analyze(x)
            x = self.decompressor(x)
        return self._tail(x)

    def update(self):
        self.bottleneck_updated = True

    def get_aux_module(self, **kwargs):
        return None


def wrap_model(wrapper_model_name, model, compression_model, **kwargs):
    if wrapper_model_name not in WRAPPER_CLASS_DICT:
        raise ValueError('wrapper_model_name `{}` is not expected'.format(wrapper_model_name))
    return WRAPPER_CLASS_DICT[wrapper_model_name](model, compression_model=compression_model, **kwargs)


def load_classification_model(model_config, device, strict=True):
    """`{key, kwargs, src_ckpt?}` -> classifier on `device` (registry.py:108-139): this build's ResNets and backbones."""
    from .backbone import get_backbone
    from .ckpt import load_ckpt
    from .resnet import RESNET_FUNC_DICT
    name = model_config['key']
    kwargs = dict(model_config.get('kwargs') or {})
    model = RESNET_FUNC_DICT[name](**kwargs) if name in RESNET_FUNC_DICT else get_backbone(name, **kwargs)
    if model is None:
        raise KeyError('classification model `{}` is not available in this build'.format(name))
    if model_config.get('src_ckpt') is not None:
        load_ckpt(model_config['src_ckpt'], model=model, strict=strict)
    return model.to(device)


def get_wrapped_classification_model(wrapper_model_config, device):
    """models.model block with a `classification_model` entry -> wrapped model (wrapper.py:343-370)."""
    from .ckpt import load_ckpt
    from .compression import get_compression_model
    name = wrapper_model_config['key']
    if name not in WRAPPER_CLASS_DICT:
        raise ValueError('wrapper_model_name `{}` is not expected'.format(name))
    compression_model = get_compression_model(wrapper_model_config.get('compression_model', None), device)
    model = load_classification_model(wrapper_model_config['classification_model'], device)
    wrapped = WRAPPER_CLASS_DICT[name](model, compression_model=compression_model, device=device,
                                       **(wrapper_model_config.get('kwargs') or {}))
    if wrapper_model_config.get('src_ckpt') is not None:
        load_ckpt(wrapper_model_config['src_ckpt'], model=wrapped, strict=False)
    return wrapped


def _load_dense_model(model_config, device, registry, kind):
    """`{key, kwargs, src_ckpt?}` -> a model of `registry` on `device` (models/{detection,segmentation}/registry.py)."""
    from .ckpt import load_ckpt
    name = model_config['key']
    if name not in registry:
        raise KeyError('{} model `{}` is not available in this build (have {})'.format(kind, name, sorted(registry)))
    model = registry[name](**dict(model_config.get('kwargs') or {}))
    if model_config.get('src_ckpt') is not None:      # (a download address upstream: `load_ckpt` looks in $SC2_PRETRAINED_DIR)
        load_ckpt(model_config['src_ckpt'], model=model, strict=False)
    return model.to(device)


def load_detection_model(model_config, device):
    from .dense import DETECTION_MODEL_FUNC_DICT
    return _load_dense_model(model_config, device, DETECTION_MODEL_FUNC_DICT, 'detection')


def load_segmentation_model(model_config, device):
    from .dense import SEGMENTATION_MODEL_FUNC_DICT
    return _load_dense_model(model_config, device, SEGMENTATION_MODEL_FUNC_DICT, 'segmentation')


def _get_wrapped_dense_model(wrapper_model_config, device, model):
    from .ckpt import load_ckpt
    from .compression import get_compression_model
    name = wrapper_model_config['key']
    if name not in WRAPPER_CLASS_DICT:
        raise ValueError('wrapper_model_name `{}` is not expected'.format(name))
    compression_model = get_compression_model(wrapper_model_config.get('compression_model', None), device)
    wrapped = WRAPPER_CLASS_DICT[name](model, compression_model=compression_model, device=device,
                                       **(wrapper_model_config.get('kwargs') or {}))
    if wrapper_model_config.get('src_ckpt') is not None:
        load_ckpt(wrapper_model_config['src_ckpt'], model=wrapped, strict=False)
    return wrapped


def get_wrapped_detection_model(wrapper_model_config, device):
    """models.model block with a `detection_model` entry -> wrapped model (sc2bench/models/detection/wrapper.py:98-122)."""
    return _get_wrapped_dense_model(wrapper_model_config, device,
                                    load_detection_model(wrapper_model_config['detection_model'], device))


def get_wrapped_segmentation_model(wrapper_model_config, device):
    """models.model block with a `segmentation_model` entry -> wrapped model (sc2bench/models/segmentation/wrapper.py:120-144)."""
    return _get_wrapped_dense_model(wrapper_model_config, device,
                                    load_segmentation_model(wrapper_model_config['segmentation_model'], device))


def load_model(model_config, device):
    """script/task/image_classification.py:52-55."""
    if 'classification_model' not in model_config:
        return load_classification_model(model_config, device)
    return get_wrapped_classification_model(model_config, device)
