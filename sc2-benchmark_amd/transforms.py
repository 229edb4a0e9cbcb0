"""Transforms the reference's configs name: the sc2bench ones (`sc2bench.transforms.codec`, `sc2bench.transforms.misc`)
and the handful of torchvision ones the BASELINE configs build with `!import_call` (torchvision is not installed in this
image; `config.resolve` maps `torchvision.transforms.<Name>` here).

* `PILTensorModule` -- sc2bench/transforms/codec.py:114-186: a feature tensor [C,H,W] goes through an image codec three
  channels at a time (config 1: JPEG quality 90, configs/ilsvrc2012/feature_compression/jpeg-resnet50.yaml:42-48).  The
  normalisation is the reference's `(x - min) / max` and `* max + min` (codec.py:159,170) -- not a min-max scaling, kept
  as is because the reported sizes and accuracies depend on it.  An f32 device tensor of at most 64 x 64 per channel with plain
  `format='JPEG'` (optional integer quality) runs on the library's kernel (csrc/jpeg.hip: one launch per batch, `forward_batch`),
  with the same features and sizes bit for bit; everything else goes through PIL as before.
* `PILImageModule` -- codec.py:79-111.  `forward_batch(images, device)` sends a list of equal-size RGB / grey images with plain
  `format='JPEG'` through the library's kernels at full image size (csrc/jpeg_image.hip, `hip.host_policy.jpeg_image_hip`), with
  the same decoded pixels and file sizes bit for bit; everything else goes through PIL image by image.
* `AdaptivePad` -- sc2bench/transforms/misc.py:105-154 (tests 'equal_side', otherwise pads right and bottom).
* `Compose`, `Resize`, `CenterCrop`, `ToTensor`, `Normalize`, `RandomResizedCrop`, `RandomHorizontalFlip` -- torchvision
  semantics on PIL images / tensors, PIL + torch only.
* `CustomCompose`, `CustomRandomResize`, `CustomRandomHorizontalFlip`, `CustomRandomCrop`, `CustomCenterCrop`, `CustomToTensor`,
  `CustomNormalize`, `pad_if_smaller` -- script/task/custom/transform.py, the (image, target) transforms of PASCAL VOC 2012
  (`CUSTOM_TRANSFORM_DICT`; `config.resolve` maps `custom.transform.<Name>` here), and misc.py's `CustomToTensor`.
  `CustomCompose.plan` records the draws of the train / evaluation chain in a `DeferredSegSample`; the collate functions pack those
  into a `DeferredSegBatch`, whose `materialize(device)` runs the whole chain on the library's kernel (csrc/seg_augment.hip,
  `hip.host_policy.seg_augment_hip`) with the host chain's tensors bit for bit, or on the host without a device.
* `DeferredClsSample` / `DeferredClsBatch` -- the planned form of an ImageNet sample and batch (`Compose.plan`, `cls_collate_fn`): the box
  of source bytes the chain's output depends on and the drawn crop / flip; `materialize(device)` finishes the batch by one copy up and
  one launch (csrc/cls_input.hip, `hip.host_policy.cls_input_hip`) with the host chain's tensors bit for bit, or on the host.
* `DeferredDetSample` / `DeferredDetBatch` -- the planned form of a COCO sample and batch (`coco_data.Compose.plan`, `coco_collate_fn`):
  source bytes and the drawn flip; `detection.GeneralizedRCNNTransform` finishes the batch on the device by one copy up and one
  launch (csrc/det_input.hip, `hip.host_policy.det_input_hip`), `tensors(device)` gives the host chain's float32 list bit for bit.
* `SimpleQuantizer` / `SimpleDequantizer` -- misc.py:181-231, the 8-bit affine quantizer of the CR+BQ baseline, with
  torchdistill's `QuantizedTensor` / `quantize_tensor` / `dequantize_tensor` (tensor_util) restated here.  On a device tensor the
  8-bit form runs on the library's kernels (csrc/bq.hip), on a CPU tensor on torch ops; both give the same bits.
Everything else runs on the host (PIL codecs are host code in the reference too): callers of the hot path, not part of it.
"""
import collections
import math
import random
from io import BytesIO

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .analysis import get_binary_object_size

CODEC_TRANSFORM_MODULE_DICT = dict()
MISC_TRANSFORM_MODULE_DICT = dict()
TORCHVISION_TRANSFORM_DICT = dict()


def register_codec_transform_module(cls):
    CODEC_TRANSFORM_MODULE_DICT[cls.__name__] = cls
    return cls


def register_misc_transform_module(cls):
    MISC_TRANSFORM_MODULE_DICT[cls.__name__] = cls
    return cls


def _tv(cls):
    TORCHVISION_TRANSFORM_DICT[cls.__name__] = cls
    return cls


# --------------------------------------------------------------------------------------------------------- functional
def _is_pil(x):
    from PIL import Image
    return isinstance(x, Image.Image)


def to_pil_image(pic):
    """float CHW in [0, 1] (-> mul(255).byte(), as torchvision: out-of-range values wrap) or uint8 CHW -> PIL L / RGB."""
    from PIL import Image
    if pic.dim() == 2:
        pic = pic.unsqueeze(0)
    if pic.is_floating_point():
        pic = pic.mul(255).byte()
    arr = np.transpose(pic.cpu().numpy(), (1, 2, 0))
    if arr.shape[2] == 1:
        return Image.fromarray(np.ascontiguousarray(arr[:, :, 0]), mode='L')
    if arr.shape[2] == 3:
        return Image.fromarray(np.ascontiguousarray(arr), mode='RGB')
    raise ValueError('to_pil_image: {} channels'.format(arr.shape[2]))


_UNIT_TABLES = dict()       # device -> f32 [256]: v / 255 as the host divides


def _u8_to_unit(pic):
    """uint8 tensor -> float32 / 255 on its device, with the host's values: there `.to(float32).div(255)` is a correctly rounded
    division, while torch's device kernel for a Python-scalar divisor multiplies by the reciprocal (one bit off for some of the 256
    values); the 256 quotients therefore come from a table built on the host."""
    if not pic.is_cuda:
        return pic.to(torch.float32).div(255)
    table = _UNIT_TABLES.get(pic.device)
    if table is None:
        with torch.inference_mode(False):
            table = _UNIT_TABLES[pic.device] = torch.arange(256, dtype=torch.float32).div(255).to(pic.device)
    return table[pic.to(torch.int32)]


def to_tensor(pic):
    """8-bit PIL image (or HWC uint8 ndarray) -> float CHW tensor / 255.  Beyond torchvision: a uint8 torch tensor [C,H,W] or
    [B,C,H,W] on any device -- decoded pixels that are on the device already (`PILImageModule.forward_batch`) -- gives the values
    of `.to(float32).div(255)` there, layout unchanged: the same as `to_tensor` of the PIL image of those pixels."""
    if isinstance(pic, torch.Tensor) and pic.dtype == torch.uint8 and pic.dim() in (3, 4):
        return _u8_to_unit(pic)
    arr = np.array(pic, copy=True)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    t = torch.from_numpy(arr).permute(2, 0, 1).contiguous()
    return t.to(torch.float32).div(255) if t.dtype == torch.uint8 else t.to(torch.float32)


def pad(x, padding, fill=0, padding_mode='constant'):
    """torchvision.transforms.functional.pad for tensors [..., H, W] and PIL images; padding = int | [lr, tb] | [l, t, r, b]."""
    if isinstance(padding, int):
        padding = [padding] * 4
    elif len(padding) == 2:
        padding = [padding[0], padding[1], padding[0], padding[1]]
    left, top, right, bottom = padding
    if _is_pil(x):
        from PIL import ImageOps
        assert padding_mode == 'constant'
        return ImageOps.expand(x, border=(left, top, right, bottom), fill=fill)
    if padding_mode == 'constant':
        return F.pad(x, [left, right, top, bottom], mode='constant', value=fill)
    return F.pad(x, [left, right, top, bottom], mode=padding_mode)


def _size_hw(x):
    if _is_pil(x):
        return x.size[1], x.size[0]
    return x.shape[-2], x.shape[-1]


# --------------------------------------------------------------------------------------------------------- torchvision
@_tv
class Compose(object):
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x

    def __repr__(self):
        return 'Compose({})'.format(self.transforms)

    def _cls_chain(self):
        """('train', crop, flip, normalize) for RandomResizedCrop -> RandomHorizontalFlip -> ToTensor -> Normalize, ('eval', resize,
        crop, normalize) for Resize -> CenterCrop -> ToTensor -> Normalize -- the two chains of configs/ilsvrc2012/** -- bilinear, with
        three-value mean / std and a Resize size that is an int or (h, w); else None."""
        ts = list(self.transforms)
        if len(ts) != 4 or type(ts[2]) is not ToTensor or type(ts[3]) is not Normalize or len(ts[3].mean) != 3 or len(ts[3].std) != 3:
            return None
        if any(float(v) == 0.0 for v in ts[3].std):
            return None
        if type(ts[0]) is RandomResizedCrop and type(ts[1]) is RandomHorizontalFlip:
            size = ts[0].size
            if ts[0].resize.interpolation != INTERPOLATION['bilinear'] or len(size) != 2 or not all(isinstance(v, int) and v >= 1 for v in size):
                return None
            return 'train', ts[0], ts[1], ts[3]
        if type(ts[0]) is Resize and type(ts[1]) is CenterCrop:
            size = ts[0].size
            pair = isinstance(size, (list, tuple)) and len(size) == 2 and all(isinstance(v, int) for v in size)
            if ts[0].interpolation != INTERPOLATION['bilinear'] or not ((isinstance(size, int) and not isinstance(size, bool)) or pair):
                return None
            if len(ts[1].size) != 2 or not all(isinstance(v, int) and v >= 1 for v in ts[1].size):
                return None
            return 'eval', ts[0], ts[1], ts[3]
        return None

    def plan(self, img):
        """One of the two ImageNet chains (`_cls_chain`) on an 8-bit RGB PIL image: draws what `__call__` would draw, in its order, and
        returns the `DeferredClsSample` -- the box of source bytes the chain's output depends on and the parameters, no pixel resampled
        (but for a sample beyond sc2_cls_input's ratio cap, which is finished here, by Pillow).  Any other chain or input, or a centre
        crop larger than the resized image (which pads): None, and nothing drawn."""
        chain = self._cls_chain()
        if chain is None or not _is_pil(img) or img.mode != 'RGB' or min(img.size) < 1:
            return None
        w, h = img.size
        if chain[0] == 'train':
            _, crop, flip, normalize = chain
            oh, ow = crop.size
            top, left, ch, cw = crop.draw(h, w)
            flipped = flip.draw()
            if ch > 4 * oh or cw > 4 * ow:       # beyond the kernel's nine taps: Pillow, here
                done = img.crop((left, top, left + cw, top + ch)).resize((ow, oh), INTERPOLATION['bilinear'])
                return DeferredClsSample.identity(_hflip(done) if flipped else done, normalize.mean, normalize.std)
            box = np.asarray(img.crop((left, top, left + cw, top + ch)))
            return DeferredClsSample(box, ch, cw, 0, 0, oh, ow, flipped, 0, 0, oh, ow, normalize.mean, normalize.std)
        _, resize, crop, normalize = chain
        oh, ow = crop.size
        nh, nw = _resized_hw(h, w, resize.size if isinstance(resize.size, int) else list(resize.size))
        if oh > nh or ow > nw:
            return None
        top, left = int(round((nh - oh) / 2.0)), int(round((nw - ow) / 2.0))
        if h > 4 * nh or w > 4 * nw:
            done = img.resize((nw, nh), INTERPOLATION['bilinear']).crop((left, top, left + ow, top + oh))
            return DeferredClsSample.identity(done, normalize.mean, normalize.std)
        (r0, r1), (c0, c1) = pil_tap_span(h, nh, top, oh), pil_tap_span(w, nw, left, ow)
        box = np.asarray(img.crop((c0, r0, c1, r1)))
        return DeferredClsSample(box, h, w, r0, c0, nh, nw, False, top, left, oh, ow, normalize.mean, normalize.std)


INTERPOLATION = {'nearest': 0, 'lanczos': 1, 'bilinear': 2, 'bicubic': 3, 'box': 4, 'hamming': 5}


@_tv
class Resize(nn.Module):
    """int size: the shorter side becomes `size` (aspect kept); (h, w): exact.  PIL images (bilinear by default)."""

    def __init__(self, size, interpolation='bilinear', **kwargs):
        super().__init__()
        self.size = size
        self.interpolation = INTERPOLATION.get(interpolation, 2) if isinstance(interpolation, str) else 2

    def forward(self, img):
        h, w = _size_hw(img)
        if isinstance(self.size, int) or len(self.size) == 1:
            s = self.size if isinstance(self.size, int) else self.size[0]
            short, long_ = (w, h) if w <= h else (h, w)
            new_short, new_long = s, int(s * long_ / short)
            nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
        else:
            nh, nw = self.size
        if _is_pil(img):
            return img.resize((nw, nh), self.interpolation)
        x = img.unsqueeze(0) if img.dim() == 3 else img
        x = F.interpolate(x.float(), size=(nh, nw), mode='bilinear', align_corners=False, antialias=True)
        return x.squeeze(0) if img.dim() == 3 else x


@_tv
class CenterCrop(nn.Module):
    def __init__(self, size):
        super().__init__()
        self.size = (size, size) if isinstance(size, int) else tuple(size)

    def forward(self, img):
        th, tw = self.size
        h, w = _size_hw(img)
        if tw > w or th > h:     # torchvision pads with zeros first
            pl, pt = max((tw - w) // 2, 0), max((th - h) // 2, 0)
            img = pad(img, [pl, pt, max((tw - w + 1) // 2, 0), max((th - h + 1) // 2, 0)])
            h, w = _size_hw(img)
        top, left = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
        if _is_pil(img):
            return img.crop((left, top, left + tw, top + th))
        return img[..., top:top + th, left:left + tw]


@_tv
class ToTensor(object):
    def __call__(self, pic):
        return to_tensor(pic)


@_tv
class Normalize(nn.Module):
    def __init__(self, mean, std, inplace=False):
        super().__init__()
        self.mean, self.std = list(mean), list(std)

    def forward(self, x):
        # (the two constant vectors live on the input's device once: building them per call is a blocking host-to-device copy,
        #  4 ms each with a busy device queue -- it was 8 of the 12 ms of a pipelined fp_input step, tools/host_prof_workload.py)
        key = (x.dtype, x.device)
        cached = self.__dict__.get('_consts')
        if cached is None or cached[0] != key or cached[3] != (tuple(self.mean), tuple(self.std)):
            # built OUTSIDE inference mode whatever the caller's mode: evaluate() runs under torch.inference_mode, and an inference
            # tensor cached there cannot be saved for backward by a later grad-mode call (codec training through
            # NeuralInputCompressionClassifier's post_transform)
            with torch.inference_mode(False):
                cached = (key, torch.as_tensor(self.mean, dtype=x.dtype, device=x.device).view(-1, 1, 1),
                          torch.as_tensor(self.std, dtype=x.dtype, device=x.device).view(-1, 1, 1), (tuple(self.mean), tuple(self.std)))
            self.__dict__['_consts'] = cached
        return (x - cached[1]) / cached[2]

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_consts', None)          # device tensors of a cache do not belong in a pickle
        return state


@_tv
class RandomHorizontalFlip(nn.Module):
    def __init__(self, p=0.5):
        super().__init__()
        self.p = p

    def draw(self):
        """True when the image is flipped: the one number `forward` draws"""
        return not random.random() >= self.p

    def forward(self, img):
        if not self.draw():
            return img
        if _is_pil(img):
            from PIL import Image
            return img.transpose(Image.FLIP_LEFT_RIGHT)
        return img.flip(-1)


@_tv
class RandomResizedCrop(nn.Module):
    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation='bilinear', **kwargs):
        super().__init__()
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.scale, self.ratio = scale, ratio
        self.resize = Resize(self.size, interpolation if interpolation is not None else 'bilinear')

    def draw(self, h, w):
        """-> (top, left, ch, cw), the crop box of an h x w image: the numbers `forward` draws, in its order"""
        area = h * w
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        top = left = 0
        ch, cw = h, w
        for _ in range(10):
            target = area * random.uniform(self.scale[0], self.scale[1])
            aspect = math.exp(random.uniform(*log_ratio))
            tw, th = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < tw <= w and 0 < th <= h:
                top, left, ch, cw = random.randint(0, h - th), random.randint(0, w - tw), th, tw
                break
        else:   # central crop at the closest valid ratio
            in_ratio = w / h
            if in_ratio < min(self.ratio):
                cw, ch = w, int(round(w / min(self.ratio)))
            elif in_ratio > max(self.ratio):
                ch, cw = h, int(round(h * max(self.ratio)))
            top, left = (h - ch) // 2, (w - cw) // 2
        return top, left, ch, cw

    def forward(self, img):
        top, left, ch, cw = self.draw(*_size_hw(img))
        img = img.crop((left, top, left + cw, top + ch)) if _is_pil(img) else img[..., top:top + ch, left:left + cw]
        return self.resize(img)


# --------------------------------------------------------------------------------------------------------- sc2bench.misc
@register_misc_transform_module
class AdaptivePad(nn.Module):
    """Pads an image tensor so that both sides become multiples of `factor` (misc.py:105-154)."""

    def __init__(self, fill=0, padding_position='hw', padding_mode='constant', factor=128, returns_org_patch_size=False):
        super().__init__()
        self.fill = fill
        self.padding_position = padding_position
        self.padding_mode = padding_mode
        self.factor = factor
        self.returns_org_patch_size = returns_org_patch_size

    def forward(self, x):
        # written against the behaviour of misc.py:141-154 (not its text): each side grows by what it lacks to the next
        # multiple of `factor`; 'equal_side' hands torchvision's two-value form HALF of that per side (so an odd remainder
        # ends one short of a multiple -- the reference's behaviour, kept), anything else pads right and bottom only
        org_h, org_w = (int(v) for v in x.shape[-2:])
        lack_h, lack_w = -org_h % self.factor, -org_w % self.factor
        if self.padding_position == 'equal_side':
            borders = [lack_w // 2, lack_h // 2]                # left = right, top = bottom
        else:
            borders = [0, 0, lack_w, lack_h]                    # left, top, right, bottom
        x = pad(x, borders, self.fill, self.padding_mode)
        return (x, (org_h, org_w)) if self.returns_org_patch_size else x


@register_misc_transform_module
class ClearTargetTransform(nn.Module):
    def forward(self, sample, *args):
        return sample, list()


# torchdistill.common.tensor_util.QuantizedTensor: module-level, so that FileSizeAnalyzer can pickle it
QuantizedTensor = collections.namedtuple('QuantizedTensor', ['tensor', 'scale', 'zero_point'])


def _nan_zero_point():
    # what the reference's `int(zero_point)` raises when the zero point is NaN (a NaN in the tensor, or an all-zero one: 0 / 0)
    raise ValueError('cannot convert float NaN to integer')


def quantize_tensor(x, num_bits=8, per_sample=False):
    """torchdistill's `quantize_tensor` (Jacob et al., asymmetric, unsigned): f32 arithmetic, in this order --
    scale = (max - min) / (2^bits - 1); zero_point = int(clamp(0 - min / scale, 0, 2^bits - 1));
    q = (zero_point + x / scale).clamp(0, 2^bits - 1).round().byte().  -> QuantizedTensor(q, scale 0-dim tensor on x's device,
    zero_point Python int).  A positive tensor therefore saturates (zero point 0): the reference's behaviour, kept.
    `per_sample=True` (not in the reference): one scale and zero point per x[i] -- what the reference's batch-size-1 evaluation
    computes for each image -- as tensors [N] (zero_point int32).
    An f32 tensor on the device with num_bits 8 runs on `hip.bq_quantize`; its one device-to-host read brings the zero point(s)
    and the status.  Everything else runs the same steps as torch ops."""
    q_max = 2.0 ** num_bits - 1.0
    if x.is_cuda and num_bits == 8 and x.dtype == torch.float32 and x.numel() > 0:
        from . import hip
        q, scale, zero_point, status = hip.bq_quantize(x.detach(), per_sample=per_sample)
        zp_host, st_host = hip.bq_read_params(zero_point, status)
        if any(st_host):
            _nan_zero_point()
        if per_sample:
            return QuantizedTensor(tensor=q, scale=scale, zero_point=zero_point)
        return QuantizedTensor(tensor=q, scale=scale.reshape(()), zero_point=zp_host[0])
    rows = x.detach().reshape(x.shape[0] if per_sample else 1, -1)
    low, high = rows.min(dim=1).values, rows.max(dim=1).values
    scale = (high - low) / q_max
    first = 0.0 - low / scale
    if bool(torch.isnan(first).any()):
        _nan_zero_point()
    zero_point = first.clamp(0.0, q_max).to(torch.int32)       # (truncation toward zero, as int())
    q = zero_point.to(rows.dtype).unsqueeze(1) + rows / scale.unsqueeze(1)
    q = q.clamp_(0.0, q_max).round_().to(torch.uint8).reshape(x.shape)
    if per_sample:
        return QuantizedTensor(tensor=q, scale=scale, zero_point=zero_point)
    return QuantizedTensor(tensor=q, scale=scale.reshape(()), zero_point=int(zero_point[0]))


def dequantize_tensor(q_x):
    """torchdistill's `dequantize_tensor`: scale * (q.float() - zero_point); takes both forms `quantize_tensor` returns."""
    q, scale, zero_point = q_x.tensor, q_x.scale, q_x.zero_point
    if q.is_cuda and q.dtype == torch.uint8 and q.numel() > 0 and isinstance(scale, torch.Tensor) and scale.is_cuda:
        from . import hip
        return hip.bq_dequantize(q, scale, zero_point)
    if isinstance(zero_point, torch.Tensor) and zero_point.dim() > 0:
        shape = (-1,) + (1,) * (q.dim() - 1)
        return scale.reshape(shape) * (q.float() - zero_point.to(q.device).reshape(shape).float())
    return scale * (q.float() - zero_point)


@register_misc_transform_module
class SimpleQuantizer(nn.Module):
    """num_bits 16: `z.half()`; num_bits 8: `quantize_tensor` (misc.py:181-205).  `per_sample` (not in the reference, default off):
    one scale per image of a batch."""

    def __init__(self, num_bits, per_sample=False):
        super().__init__()
        self.num_bits = num_bits
        self.per_sample = per_sample

    def forward(self, z):
        return z.half() if self.num_bits == 16 else quantize_tensor(z, self.num_bits, per_sample=self.per_sample)


@register_misc_transform_module
class SimpleDequantizer(nn.Module):
    """num_bits 16: `z.float()`; else `dequantize_tensor` (misc.py:208-231)."""

    def __init__(self, num_bits):
        super().__init__()
        self.num_bits = num_bits

    def forward(self, z):
        return z.float() if self.num_bits == 16 else dequantize_tensor(z)


def default_collate_w_pil(batch):
    """torchdistill's `default_collate_w_pil`: like default_collate, but PIL images are kept as a list."""
    from torch.utils.data import default_collate
    elem = batch[0]
    if _is_pil(elem):
        return list(batch)
    if isinstance(elem, (tuple, list)):
        return [default_collate_w_pil(list(samples)) for samples in zip(*batch)]
    return default_collate(batch)


# ------------------------------------------------------------------------------------- sc2bench.transforms.collator
def cat_list(images, fill_value=0):
    """Tensors of different sizes -> one batch tensor of the largest size along every dimension, each sample in its top-left
    corner, the rest `fill_value` (dtype and device of the first sample).  A single sample that is not a tensor (a PIL image
    at batch size 1) is handed back as it came."""
    if len(images) == 1 and not isinstance(images[0], torch.Tensor):
        return images
    shape = tuple(max(dims) for dims in zip(*(img.shape for img in images)))
    batch = images[0].new_full((len(images),) + shape, fill_value)
    for i, img in enumerate(images):
        batch[i][..., :img.shape[-2], :img.shape[-1]].copy_(img)
    return batch


COLLATE_FUNC_DICT = dict()


def register_collate_func(func):
    COLLATE_FUNC_DICT[func.__name__] = func
    return func


register_collate_func(default_collate_w_pil)


@register_collate_func
def pascal_seg_collate_fn(batch):
    """(image, target, supplementary dict) triplets of PASCAL VOC 2012 -> (images padded with 0, targets padded with the ignore
    label 255, the dicts as a tuple).  Triplets whose first item is a `DeferredSegSample` (its target slot is ignored) -> one
    `DeferredSegBatch` with the dicts in `.extra[0]`."""
    deferred = _collate_deferred(batch, True)
    if deferred is not None:
        return deferred
    images, targets, supp_dicts = zip(*batch)
    return cat_list(images, fill_value=0), cat_list(targets, fill_value=255), supp_dicts


@register_collate_func
def pascal_seg_eval_collate_fn(batch):
    """(image, target) pairs -> (images padded with 0, targets padded with 255); pairs whose first item is a `DeferredSegSample` ->
    one `DeferredSegBatch`."""
    deferred = _collate_deferred(batch, False)
    if deferred is not None:
        return deferred
    images, targets = zip(*batch)
    return cat_list(images, fill_value=0), cat_list(targets, fill_value=255)


@register_collate_func
def coco_collate_fn(batch):
    """(image, target dict) pairs of COCO 2017 -> (images as a tuple, targets as a tuple): detection batches are lists, never padded
    (every `configs/coco2017/**` loader names it).  Pairs whose first item is a `DeferredDetSample` -> (one `DeferredDetBatch`, targets
    as a tuple); a batch that mixes planned and transformed samples raises TypeError."""
    firsts = [item[0] for item in batch]
    if any(isinstance(f, DeferredDetSample) for f in firsts):
        if not all(isinstance(f, DeferredDetSample) for f in firsts):
            raise TypeError('a batch mixes planned and transformed samples')
        return DeferredDetBatch(firsts), tuple(item[1] for item in batch)
    return tuple(zip(*batch))


# --------------------------------------------------------------------------------------------------------- sc2bench.codec
def _pil_codec_round_trip(pil_img, save_kwargs, open_kwargs):
    """image -> codec bytes in memory -> reopened image: (image, byte count of the coded file)."""
    from PIL import Image
    coded = BytesIO()
    pil_img.save(coded, **save_kwargs)
    n_bytes = coded.tell()          # before reopening: the decoder moves the position
    return Image.open(coded, **open_kwargs), n_bytes


def _plain_jpeg_quality(save_kwargs, open_kwargs):
    """The quality when `save_kwargs` / `open_kwargs` ask for nothing but `format='JPEG'` at an integer quality (Pillow's default
    is 75) -- the one case the kernels restate --, else None: `optimize`, `subsampling`, `progressive`, other formats stay with PIL."""
    kw = save_kwargs
    if open_kwargs or set(kw) - {'format', 'quality'} or not isinstance(kw.get('format'), str) or kw['format'].upper() != 'JPEG':
        return None
    quality = kw.get('quality', 75)
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        return None
    return quality


@register_codec_transform_module
class PILImageModule(nn.Module):
    """Compresses (and reopens) a PIL image with a PIL codec (codec.py:79-111).  `forward_batch` takes a list of images: equal-size
    RGB / grey ones with plain `format='JPEG'` go up in one copy and through the library's kernels (csrc/jpeg_image.hip) when
    `hip.host_policy.jpeg_image_hip` is on, with the same pixels and sizes; everything else goes through PIL image by image."""

    def __init__(self, returns_file_size=False, open_kwargs=None, **save_kwargs):
        super().__init__()
        self.returns_file_size = returns_file_size
        self.open_kwargs = open_kwargs if isinstance(open_kwargs, dict) else dict()
        self.save_kwargs = save_kwargs

    def forward(self, pil_img, *args):
        decoded, n_bytes = _pil_codec_round_trip(pil_img, self.save_kwargs, self.open_kwargs)
        return (decoded, n_bytes) if self.returns_file_size else decoded

    def _jpeg_quality(self):
        """The gate in front of the kernel, shared with `PILTensorModule`: the quality of plain `format='JPEG'`, else None."""
        return _plain_jpeg_quality(self.save_kwargs, self.open_kwargs)

    def _kernel_quality(self, images, device):
        """The quality when this list of PIL images goes to the kernel on `device`, else None: a HIP device, plain JPEG, one size and
        one mode ('RGB' or 'L') for all, sides within the kernel's limit, and no image with a 'comment' in its `.info` -- Pillow's JPEG
        writer copies that into a COM segment (ImageNet files carry such comments through convert / resize / crop), so such a batch
        has to report Pillow's size."""
        quality = self._jpeg_quality()
        if quality is None or len(images) == 0 or torch.device(device).type != 'cuda':
            return None
        first = images[0]
        if not _is_pil(first) or first.mode not in ('RGB', 'L'):
            return None
        for img in images:
            if not _is_pil(img) or img.size != first.size or img.mode != first.mode or 'comment' in img.info:
                return None
        from . import hip
        if not hip.host_policy.jpeg_image_hip or max(first.size) > hip.JPEG_IMAGE_MAX_SIDE or min(first.size) < 1:
            return None
        return quality

    def forward_batch(self, images, device):
        """images: list of PIL images -> (decoded, [file size of every image]): what `forward` (with `returns_file_size`) gives image
        by image.  On the kernel path `decoded` is the uint8 device tensor [B,C,H,W] of the decoded pixels (one host-to-device copy of
        the stacked images, one device-to-host read of the sizes), otherwise the list of reopened PIL images."""
        quality = self._kernel_quality(images, device)
        if quality is None:
            pairs = [_pil_codec_round_trip(img, self.save_kwargs, self.open_kwargs) for img in images]
            return [d for d, _ in pairs], [n for _, n in pairs]
        from . import hip, jpeg_format
        mode, (W, H) = images[0].mode, images[0].size
        # (the kernel counts whole files; the header length it adds is the one Pillow writes at this size and quality)
        kernel_mode = hip.JPEG_RGB if mode == 'RGB' else hip.JPEG_GREY
        if jpeg_format.checked_header_bytes(mode, H, W, quality) != hip.JPEG_HEADER_BYTES[kernel_mode]:
            raise hip.Sc2Error('jpeg header of {} bytes expected for mode {}'.format(hip.JPEG_HEADER_BYTES[kernel_mode], mode))
        stacked = torch.from_numpy(np.stack([np.asarray(img) for img in images]))              # [B,H,W,3] or [B,H,W]
        stacked = stacked.to(device, non_blocking=True)
        x = stacked.permute(0, 3, 1, 2) if mode == 'RGB' else stacked.unsqueeze(1)             # read in place: no layout pass
        res = hip.jpeg_image_codec(x, quality)
        return res.recon, res.sizes.cpu().tolist()

    def __repr__(self):
        return self.__class__.__name__ + '(returns_file_size={}, open_kwargs={}, save_kwargs={})'.format(
            self.returns_file_size, self.open_kwargs, self.save_kwargs)


@register_codec_transform_module
class PILTensorModule(nn.Module):
    """Compresses (and reconstructs) a tensor [C,H,W] with a PIL codec, three channels per image (codec.py:114-186)."""

    def __init__(self, returns_file_size=False, open_kwargs=None, **save_kwargs):
        super().__init__()
        self.returns_file_size = returns_file_size
        self.open_kwargs = open_kwargs if isinstance(open_kwargs, dict) else dict()
        self.save_kwargs = save_kwargs

    @staticmethod
    def _channel_groups(x):
        """[C,H,W] -> groups of three channels (RGB images); a remainder of one goes as a grey image, a remainder of two as
        two grey images (a two-channel tensor has no PIL mode)."""
        groups = list(x.split(3, dim=0))
        if groups[-1].shape[0] == 2:
            groups[-1:] = list(groups[-1].split(1, dim=0))
        return groups

    def _forward_host(self, x, with_size):
        # written against the behaviour of codec.py:141-186: per channel group, scale with the group's own extrema AS THE
        # REFERENCE DOES -- (v - min) / max on the way in, v * max + min on the way out, which is not a min-max scaling and
        # must not be "fixed"  --, 8-bit image through the codec, back to a tensor on x's device.  The
        # payload is the coded images plus the two pickled lists of 0-dim tensors the receiver needs to undo the scaling.
        lows, highs, restored, coded_bytes = [], [], [], 0
        for group in self._channel_groups(x):
            high, low = group.max(), group.min()
            decoded, n_bytes = _pil_codec_round_trip(to_pil_image((group - low) / high), self.save_kwargs, self.open_kwargs)
            coded_bytes += n_bytes
            if group.shape[0] == 1 and decoded.mode != 'L':     # a grey image some codecs reopen as RGB
                decoded = decoded.convert('L')
            restored.append(to_tensor(decoded).to(x.device) * high + low)
            lows.append(low)
            highs.append(high)
        features = torch.vstack(restored)
        if not with_size:
            return features
        side_info = get_binary_object_size(lows, unit_size=1) + get_binary_object_size(highs, unit_size=1)
        return features, coded_bytes + side_info

    # ---- baseline JPEG of an f32 device tensor: one launch for the whole batch (csrc/jpeg.hip)
    _side_info_cache = dict()

    def _jpeg_quality(self):
        """The gate in front of the kernel, shared with `PILImageModule`: the quality of plain `format='JPEG'`, else None."""
        return _plain_jpeg_quality(self.save_kwargs, self.open_kwargs)

    def _kernel_quality(self, x):
        """The quality when x [..., C,H,W] goes to the kernel, else None."""
        quality = self._jpeg_quality()
        if quality is None or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.numel() == 0:
            return None
        from . import hip
        if x.shape[-1] > hip.JPEG_MAX_SIDE or x.shape[-2] > hip.JPEG_MAX_SIDE or not hip.host_policy.jpeg_codec_hip:
            return None
        return quality

    @classmethod
    def _side_info_bytes(cls, n, dtype, device):
        """What the host path adds for the two pickled lists of n 0-dim extrema on `device`: the pickle's length depends on n, dtype
        and device, not on the values, so it is measured once per key on real 0-dim tensors."""
        key = (n, dtype, str(device))
        if key not in cls._side_info_cache:
            scalars = [torch.zeros((), dtype=dtype, device=device) for _ in range(n)]
            cls._side_info_cache[key] = 2 * get_binary_object_size(scalars, unit_size=1)
        return cls._side_info_cache[key]

    def _forward_kernel(self, x, quality):
        """x [B,C,H,W] on the device -> (features [B,C,H,W], [size per sample]): one launch, one device-to-host read (sizes and status
        words).  A sample with a group the kernel leaves alone (negative minimum, all zero, NaN / infinity) takes the host path."""
        from . import hip, jpeg_format
        res = hip.jpeg_tensor_codec(x, quality)
        B, C, H, W = (int(v) for v in x.shape)
        n_rgb, n_grey = C // 3, C % 3
        n = n_rgb + n_grey
        meta = res.meta.cpu().reshape(2, B, n)
        # (the kernel counts whole files; the header length it adds is the one Pillow writes at this size and quality)
        for count, mode, kernel_mode in ((n_rgb, 'RGB', hip.JPEG_RGB), (n_grey, 'L', hip.JPEG_GREY)):
            if count and jpeg_format.checked_header_bytes(mode, H, W, quality) != hip.JPEG_HEADER_BYTES[kernel_mode]:
                raise hip.Sc2Error('jpeg header of {} bytes expected for mode {}'.format(hip.JPEG_HEADER_BYTES[kernel_mode], mode))
        side_info = self._side_info_bytes(n, x.dtype, x.device)
        features, sizes = res.recon, []
        for b in range(B):
            if bool(meta[1, b].any()):
                restored, size = self._forward_host(x[b], True)
                features[b] = restored
                sizes.append(size)
            else:
                sizes.append(int(meta[0, b].sum()) + side_info)
        return features, sizes

    def forward(self, x, *args):
        quality = self._kernel_quality(x) if isinstance(x, torch.Tensor) and x.dim() == 3 else None
        if quality is None:
            return self._forward_host(x, self.returns_file_size)
        features, sizes = self._forward_kernel(x.unsqueeze(0), quality)
        return (features[0], sizes[0]) if self.returns_file_size else features[0]

    def forward_batch(self, x):
        """x [B,C,H,W] -> (features [B,C,H,W], [file size of every sample]): what `forward` gives sample by sample."""
        assert x.dim() == 4
        quality = self._kernel_quality(x)
        if quality is not None:
            return self._forward_kernel(x, quality)
        pairs = [self._forward_host(sample, True) for sample in x]
        return torch.stack([f for f, _ in pairs]), [size for _, size in pairs]

    def __repr__(self):
        return self.__class__.__name__ + '(returns_file_size={}, open_kwargs={}, save_kwargs={})'.format(
            self.returns_file_size, self.open_kwargs, self.save_kwargs)


# ----------------------------------------------------------------------------------------- custom.transform (PASCAL VOC)
# script/task/custom/transform.py of the reference, restated under its names: transforms of (image, target) PAIRS.  The random draws
# come from the reference's generators in the reference's order: `random.randint` (resize), `random.random` (flip), `torch.randint`
# twice (crop), so a seeded run draws what the reference draws.
def _resized_hw(h, w, size):
    """torchvision's `resize` size rule (the one `Resize` above uses): int -> the short side becomes `size`, the long side
    int(size * long / short); [h, w] -> exact."""
    if isinstance(size, int):
        short, long_ = (w, h) if w <= h else (h, w)
        new_short, new_long = size, int(size * long_ / short)
        return (new_long, new_short) if w <= h else (new_short, new_long)
    return int(size[0]), int(size[1])


def _resize_to(x, nh, nw, nearest):
    if _is_pil(x):
        return x.resize((nw, nh), 0 if nearest else 2)
    t = x.reshape((1,) * (4 - x.dim()) + tuple(x.shape))
    if nearest:
        out = F.interpolate(t.float(), size=(nh, nw), mode='nearest').to(x.dtype)
    else:
        out = F.interpolate(t.float(), size=(nh, nw), mode='bilinear', align_corners=False, antialias=True)
    return out.reshape(tuple(x.shape[:-2]) + (nh, nw))


def _hflip(x):
    if _is_pil(x):
        from PIL import Image
        return x.transpose(Image.FLIP_LEFT_RIGHT)
    return x.flip(-1)


def _crop(x, top, left, height, width):
    if _is_pil(x):
        return x.crop((left, top, left + width, top + height))
    return x[..., top:top + height, left:left + width]


def random_crop_params(h, w, th, tw):
    """torchvision's `RandomCrop.get_params` for an h x w image and a th x tw crop -> (top, left).  [recalled: torchvision is not
    installed here] it raises when the crop is larger than the image, draws NOTHING when the image is exactly th x tw, and otherwise
    draws `torch.randint(0, h - th + 1, (1,)).item()` and then `torch.randint(0, w - tw + 1, (1,)).item()`."""
    if h < th or w < tw:
        raise ValueError('Required crop size {} is larger than input image size {}'.format((th, tw), (h, w)))
    if w == tw and h == th:
        return 0, 0
    top = torch.randint(0, h - th + 1, size=(1,)).item()
    left = torch.randint(0, w - tw + 1, size=(1,)).item()
    return top, left


def pad_if_smaller(img, size, fill=0):
    """Pads right and bottom so that both sides reach `size` (transform.py:27-34)."""
    h, w = _size_hw(img)
    if min(h, w) < size:
        img = pad(img, [0, 0, size - w if w < size else 0, size - h if h < size else 0], fill=fill)
    return img


CUSTOM_TRANSFORM_DICT = dict()


def register_custom_transform(cls):
    CUSTOM_TRANSFORM_DICT[cls.__name__] = cls
    return cls


@register_custom_transform
class CustomRandomResize(object):
    """Short side -> random.randint(min_size, max_size) (both sides when `square`), the image bilinear, the target nearest;
    `jpeg_quality`: the image goes through Pillow's JPEG first, on the host."""

    def __init__(self, min_size, max_size=None, square=False, jpeg_quality=None):
        self.min_size = min_size
        self.max_size = min_size if max_size is None else max_size
        self.square = square
        self.jpeg_quality = jpeg_quality

    def draw(self):
        size = random.randint(self.min_size, self.max_size)
        return [size, size] if self.square else size

    def __call__(self, image, target):
        if self.jpeg_quality is not None:
            from PIL import Image
            coded = BytesIO()
            image.save(coded, 'JPEG', quality=self.jpeg_quality)
            image = Image.open(coded)
        nh, nw = _resized_hw(*_size_hw(image), self.draw())
        return _resize_to(image, nh, nw, False), _resize_to(target, nh, nw, True)


@register_custom_transform
class CustomRandomHorizontalFlip(object):
    def __init__(self, p):
        self.p = p

    def draw(self):
        return random.random() < self.p

    def __call__(self, image, target):
        if self.draw():
            image, target = _hflip(image), _hflip(target)
        return image, target


@register_custom_transform
class CustomRandomCrop(object):
    """`pad_if_smaller` (image 0, target 255), then a random size x size crop at `random_crop_params`."""

    def __init__(self, size):
        self.size = size

    def __call__(self, image, target):
        image = pad_if_smaller(image, self.size)
        target = pad_if_smaller(target, self.size, fill=255)
        top, left = random_crop_params(*_size_hw(image), self.size, self.size)
        return _crop(image, top, left, self.size, self.size), _crop(target, top, left, self.size, self.size)


@register_custom_transform
class CustomCenterCrop(object):
    def __init__(self, size):
        self.size = size
        self._crop = CenterCrop(size)

    def __call__(self, image, target):
        return self._crop(image), self._crop(target)


def _pair_to_tensor(image, target, converts_sample=True, converts_target=True):
    if converts_sample:
        image = to_tensor(image)
    if converts_target:
        target = torch.as_tensor(np.array(target), dtype=torch.int64)
    return image, target


@register_custom_transform
@register_misc_transform_module
class CustomToTensor(nn.Module):
    """Both `custom.transform.CustomToTensor` (no arguments) and `sc2bench.transforms.misc.CustomToTensor` (misc.py:158-178): ToTensor of
    the sample and / or `as_tensor(int64)` of the target."""

    def __init__(self, converts_sample=True, converts_target=True):
        super().__init__()
        self.converts_sample = converts_sample
        self.converts_target = converts_target

    def forward(self, image, target):
        return _pair_to_tensor(image, target, self.converts_sample, self.converts_target)


@register_custom_transform
class CustomNormalize(object):
    def __init__(self, mean, std):
        self.mean, self.std = list(mean), list(std)
        self._normalize = Normalize(mean, std)

    def __call__(self, image, target):
        return self._normalize(image), target


class _PlannedSample(object):
    """A planned sample pickles as the dict of its slots (a data-loader worker sends it to the main process)."""
    __slots__ = ()

    def __getstate__(self):
        return {k: getattr(self, k) for k in self.__slots__}

    def __setstate__(self, state):
        for k, v in state.items():
            setattr(self, k, v)


def _pack_planned(samples, parts_of, row_of):
    """(buf, desc) of a planned batch: the byte arrays `parts_of(sample)` of every sample back to back in one flat CPU uint8 tensor,
    and the stacked descriptor rows `row_of(sample, offset)`, offset being where the sample's bytes start"""
    rows, chunks, offset = [], [], 0
    for s in samples:
        parts = [np.ascontiguousarray(p).reshape(-1) for p in parts_of(s)]
        rows.append(row_of(s, offset))
        chunks += parts
        offset += sum(p.size for p in parts)
    return torch.from_numpy(np.concatenate(chunks)), torch.from_numpy(np.stack(rows))


def _launch_on_copy(host_buf, device, copies, launch):
    """-> launch(buf), buf being the copy of `host_buf` on the HIP device (made here unless `copies`, device -> copy, has it)"""
    with torch.cuda.device(device):         # (the launches go to the current device's current stream)
        buf = copies.get(device)
        if buf is None:
            buf = copies[device] = host_buf.to(device, non_blocking=True)
        out = launch(buf)
        # (the kernels read `buf` on the current stream: the allocator must not hand its block out before they have run)
        buf.record_stream(torch.cuda.current_stream(device))
    return out


def _planned_on_device(cls, batch, device, enabled, launch):
    """The device path of `materialize` of a planned batch: one copy up of `batch.buf`, `launch(buf)`, one read-back of the status
    words.  -> what `launch` returned; None where the host path is to be taken: no HIP device, the switch off, or a status word set
    (a sample the kernels' own checks refuse), which `cls.fallbacks` counts."""
    if device.type != 'cuda' or not enabled:
        return None
    res = _launch_on_copy(batch.buf, device, dict(), launch)
    if bool(res.status.cpu().any()):
        cls.fallbacks += 1
        return None
    return res


class DeferredSegSample(_PlannedSample):
    """What `CustomCompose.plan` hands out in place of the transformed pair: the source bytes and every drawn parameter, as numpy, so
    that a data-loader worker neither resizes nor opens the device.  image uint8 [h,w,3], mask uint8 [h,w]; (nh, nw) the resized
    size, flip, (top, left) the crop's origin in the padded, flipped, resized image, (out_h, out_w) the size of the finished
    tensors, (pad_h, pad_w) that of the padded image, mean / std of the normalisation."""
    __slots__ = ('image', 'mask', 'nh', 'nw', 'flip', 'top', 'left', 'out_h', 'out_w', 'pad_h', 'pad_w', 'mean', 'std')

    def __init__(self, image, mask, nh, nw, flip, top, left, out_h, out_w, pad_h, pad_w, mean, std):
        self.image, self.mask = image, mask
        self.nh, self.nw, self.flip, self.top, self.left = int(nh), int(nw), bool(flip), int(top), int(left)
        self.out_h, self.out_w, self.pad_h, self.pad_w = int(out_h), int(out_w), int(pad_h), int(pad_w)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)

    def host(self):
        """The pair `CustomCompose.__call__` returns for these draws: Pillow and torch on the host."""
        from PIL import Image
        image, target = Image.fromarray(self.image), Image.fromarray(self.mask)
        image, target = _resize_to(image, self.nh, self.nw, False), _resize_to(target, self.nh, self.nw, True)
        if self.flip:
            image, target = _hflip(image), _hflip(target)
        if (self.pad_h, self.pad_w) != (self.nh, self.nw):
            image = pad(image, [0, 0, self.pad_w - self.nw, self.pad_h - self.nh], fill=0)
            target = pad(target, [0, 0, self.pad_w - self.nw, self.pad_h - self.nh], fill=255)
        if (self.top, self.left, self.out_h, self.out_w) != (0, 0, self.pad_h, self.pad_w):
            image = _crop(image, self.top, self.left, self.out_h, self.out_w)
            target = _crop(target, self.top, self.left, self.out_h, self.out_w)
        image, target = _pair_to_tensor(image, target)
        return Normalize(self.mean, self.std)(image), target


@register_custom_transform
class CustomCompose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, image, target):
        for t in self.transforms:
            image, target = t(image, target)
        return image, target

    def _chain(self):
        """(resize, flip or None, crop or None, normalize) when the transforms are CustomRandomResize (no jpeg_quality) -> [flip] -> [crop]
        -> a CustomToTensor converting both -> CustomNormalize, else None."""
        ts = list(self.transforms)
        if len(ts) < 3 or not isinstance(ts[0], CustomRandomResize) or ts[0].jpeg_quality is not None:
            return None
        if not isinstance(ts[-1], CustomNormalize) or not isinstance(ts[-2], CustomToTensor):
            return None
        if not (ts[-2].converts_sample and ts[-2].converts_target) or len(ts[-1].mean) != 3 or len(ts[-1].std) != 3:
            return None
        middle = ts[1:-2]
        flip = middle.pop(0) if middle and isinstance(middle[0], CustomRandomHorizontalFlip) else None
        crop = middle.pop(0) if middle and isinstance(middle[0], CustomRandomCrop) else None
        if middle or (crop is not None and not isinstance(crop.size, int)):
            return None
        return ts[0], flip, crop, ts[-1]

    def plan(self, image, target):
        """The PASCAL train chain (resize -> [flip] -> [crop] -> ToTensor -> Normalize) or its evaluation form on an 8-bit RGB image
        and an 8-bit single-channel mask of one size: draws what `__call__` would draw, in its order, and returns the
        `DeferredSegSample` -- no pixel is touched.  Any other chain or input: None (and nothing drawn)."""
        chain = self._chain()
        if chain is None or not _is_pil(image) or not _is_pil(target) or image.mode != 'RGB' or target.mode not in ('L', 'P') or \
                image.size != target.size or min(image.size) < 1:
            return None
        resize, flip, crop, normalize = chain
        w, h = image.size
        nh, nw = _resized_hw(h, w, resize.draw())
        if nh < 1 or nw < 1:
            return None
        flipped = flip.draw() if flip is not None else False
        pad_h, pad_w, out_h, out_w, top, left = nh, nw, nh, nw, 0, 0
        if crop is not None:
            pad_h, pad_w, out_h, out_w = max(nh, crop.size), max(nw, crop.size), crop.size, crop.size
            top, left = random_crop_params(pad_h, pad_w, out_h, out_w)
        return DeferredSegSample(np.asarray(image), np.asarray(target), nh, nw, flipped, top, left, out_h, out_w, pad_h, pad_w,
                                 normalize.mean, normalize.std)


class DeferredSegBatch(object):
    """A batch of `DeferredSegSample`s as the collate functions pack it: `buf`, one flat CPU uint8 tensor with every image and mask;
    `desc`, the int32 descriptor table of `hip.seg_augment` [n, 16]; `size`, the (height, width) of the batch (the largest sample's);
    mean / std; `extra`, whatever else the collate function returns behind (images, targets).  `materialize(device)` gives the two
    tensors the host transforms and the collate function would have given -- on a HIP device with `hip.host_policy.seg_augment_hip`
    on by one copy up and sc2_seg_augment, otherwise by the host transforms with the recorded draws."""
    fallbacks = 0       # batches a status word sent back to the host path (process-wide, for the tests and the tools)

    def __init__(self, samples, extra=()):
        assert len(samples) >= 1 and all(isinstance(s, DeferredSegSample) for s in samples)
        if any((s.mean, s.std) != (samples[0].mean, samples[0].std) for s in samples):
            raise ValueError('DeferredSegBatch: samples of different normalisations')
        from . import hip
        self.mean, self.std = samples[0].mean, samples[0].std
        self.size = (max(s.out_h for s in samples), max(s.out_w for s in samples))
        self.extra = tuple(extra)
        self.buf, self.desc = _pack_planned(samples, lambda s: (s.image, s.mask), lambda s, offset: hip.seg_augment_desc(
            image_offset=offset, mask_offset=offset + s.image.size, h=s.mask.shape[0], w=s.mask.shape[1], nh=s.nh, nw=s.nw, flip=int(s.flip),
            top=s.top, left=s.left, ext_h=s.out_h, ext_w=s.out_w, pad_h=s.pad_h, pad_w=s.pad_w))

    def __len__(self):
        return int(self.desc.shape[0])

    def samples(self):
        """The `DeferredSegSample`s again, as views of `buf`."""
        out, buf = [], self.buf.numpy()
        for row in self.desc.tolist():
            io, mo, h, w, nh, nw, flip, top, left, eh, ew, ph, pw = row[:13]
            out.append(DeferredSegSample(buf[io:io + 3 * h * w].reshape(h, w, 3), buf[mo:mo + h * w].reshape(h, w), nh, nw, flip, top, left,
                                         eh, ew, ph, pw, self.mean, self.std))
        return out

    def materialize_host(self, device=None):
        pairs = [s.host() for s in self.samples()]
        images, targets = cat_list([p[0] for p in pairs], fill_value=0), cat_list([p[1] for p in pairs], fill_value=255)
        if device is not None:
            images, targets = images.to(device, non_blocking=True), targets.to(device, non_blocking=True)
        return images, targets

    def materialize(self, device=None):
        """-> (images f32 [n,3,H,W], targets int64 [n,H,W]) on `device`."""
        from . import hip
        device = torch.device('cpu' if device is None else device)
        res = _planned_on_device(DeferredSegBatch, self, device, hip.host_policy.seg_augment_hip,
                                 lambda buf: hip.seg_augment(buf, self.desc, self.size, self.mean, self.std))
        return self.materialize_host(device) if res is None else (res.images, res.targets)

    def pin_memory(self):
        self.buf = self.buf.pin_memory()
        return self


def _collate_deferred(batch, with_supp):
    """A batch of planned samples -> the tuple the collate function returns, with one DeferredSegBatch in place of (images, targets)."""
    firsts = [item[0] for item in batch]
    if not any(isinstance(f, DeferredSegSample) for f in firsts):
        return None
    if not all(isinstance(f, DeferredSegSample) for f in firsts):
        raise TypeError('a batch mixes planned and transformed samples')
    return DeferredSegBatch(firsts, extra=(tuple(item[2] for item in batch),) if with_supp else ())


def pil_tap_bounds(n_in, n_out, xx):
    """(first, count) of the source indices Pillow's bilinear resample of an axis n_in -> n_out reads for output index xx: float64,
    every operation rounded once (tests/ref_pil_resize.py proves the rule against Pillow).  An axis of equal lengths is the pass
    Pillow skips: the pixel itself."""
    if n_in == n_out:
        return xx, 1
    scale = n_in / n_out
    support = max(scale, 1.0)
    center = (xx + 0.5) * scale
    first = max(int(center - support + 0.5), 0)
    return first, min(int(center + support + 0.5), n_in) - first


def pil_tap_span(n_in, n_out, origin, length):
    """[lo, hi): the source indices the outputs origin .. origin + length - 1 read (the bounds do not decrease with the index)"""
    last = pil_tap_bounds(n_in, n_out, origin + length - 1)
    return pil_tap_bounds(n_in, n_out, origin)[0], last[0] + last[1]


class DeferredClsSample(_PlannedSample):
    """What `Compose.plan` hands out in place of the transformed image: `image`, uint8 [h,w,3], a box of the source at (row0, col0) of
    a full_h x full_w image -- the only bytes the output depends on -- and the parameters: (nh, nw) the resized size of the FULL image,
    flip, (top, left) the origin of the out_h x out_w window in the resized, flipped image, mean / std.  Train form: the box is the
    drawn crop and full = its size (Pillow clamps at the crop's edges).  Evaluation form: full is the whole image and the box the rows
    and columns the window's taps read.  A data-loader worker neither resamples nor opens the device."""
    __slots__ = ('image', 'full_h', 'full_w', 'row0', 'col0', 'nh', 'nw', 'flip', 'top', 'left', 'out_h', 'out_w', 'mean', 'std')

    def __init__(self, image, full_h, full_w, row0, col0, nh, nw, flip, top, left, out_h, out_w, mean, std):
        assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3, 'DeferredClsSample: uint8 [h,w,3] is required'
        self.image = image
        self.full_h, self.full_w, self.row0, self.col0 = int(full_h), int(full_w), int(row0), int(col0)
        self.nh, self.nw, self.flip, self.top, self.left = int(nh), int(nw), bool(flip), int(top), int(left)
        self.out_h, self.out_w = int(out_h), int(out_w)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)

    @classmethod
    def identity(cls, window, mean, std):
        """The sample of a finished 8-bit window (PIL RGB or uint8 [h,w,3]): nothing is left to resample, flip or crop."""
        window = np.asarray(window)
        h, w = window.shape[:2]
        return cls(window, h, w, 0, 0, h, w, False, 0, 0, h, w, mean, std)

    def host(self):
        """The tensor `Compose.__call__` returns for these draws: Pillow and torch on the host.  A box smaller than its full image is
        laid into a canvas of that size first: no tap of the window reads the canvas outside the box."""
        from PIL import Image
        h, w = self.image.shape[:2]
        if (h, w) == (self.full_h, self.full_w):
            image = Image.fromarray(np.ascontiguousarray(self.image))
        else:
            canvas = np.zeros((self.full_h, self.full_w, 3), np.uint8)
            canvas[self.row0:self.row0 + h, self.col0:self.col0 + w] = self.image
            image = Image.fromarray(canvas)
        if (self.nh, self.nw) != (self.full_h, self.full_w):
            image = image.resize((self.nw, self.nh), INTERPOLATION['bilinear'])
        if self.flip:
            image = _hflip(image)
        if (self.top, self.left, self.out_h, self.out_w) != (0, 0, self.nh, self.nw):
            image = _crop(image, self.top, self.left, self.out_h, self.out_w)
        return Normalize(self.mean, self.std)(to_tensor(image))


class DeferredClsBatch(object):
    """A batch of `DeferredClsSample`s as `cls_collate_fn` packs it: `buf`, one flat CPU uint8 tensor with every stored box back to
    back; `desc`, the int32 descriptor table of `hip.cls_input` [n, 16]; `size`, the (height, width) every sample ends at; mean / std.
    `to(device)` only records where the batch is wanted.  `materialize(device)` gives the float32 [n,3,H,W] batch the host transforms
    and `default_collate` would have given, bit for bit -- on a HIP device with `hip.host_policy.cls_input_hip` on by one copy up of
    `buf`, one sc2_cls_input launch and one read-back of the status words, otherwise (or when a status word is set) by the host
    transforms with the recorded draws."""
    fallbacks = 0       # batches a status word sent back to the host path (process-wide, for the tests and the tools)

    def __init__(self, samples):
        assert len(samples) >= 1 and all(isinstance(s, DeferredClsSample) for s in samples)
        first = samples[0]
        if any((s.mean, s.std) != (first.mean, first.std) for s in samples):
            raise ValueError('DeferredClsBatch: samples of different normalisations')
        if any((s.out_h, s.out_w) != (first.out_h, first.out_w) for s in samples):
            raise ValueError('DeferredClsBatch: samples of different output sizes')
        from . import hip
        self.mean, self.std, self.size = first.mean, first.std, (first.out_h, first.out_w)
        self.device = torch.device('cpu')
        self.buf, self.desc = _pack_planned(samples, lambda s: (s.image,), lambda s, offset: hip.cls_input_desc(
            offset=offset, h=s.image.shape[0], w=s.image.shape[1], full_h=s.full_h, full_w=s.full_w, row0=s.row0, col0=s.col0, nh=s.nh,
            nw=s.nw, flip=int(s.flip), top=s.top, left=s.left))

    def __len__(self):
        return int(self.desc.shape[0])

    def samples(self):
        """The `DeferredClsSample`s again, as views of `buf`."""
        out, buf = [], self.buf.numpy()
        for row in self.desc.tolist():
            off, h, w, fh, fw, row0, col0, nh, nw, flip, top, left = row[:12]
            out.append(DeferredClsSample(buf[off:off + 3 * h * w].reshape(h, w, 3), fh, fw, row0, col0, nh, nw, flip, top, left,
                                         self.size[0], self.size[1], self.mean, self.std))
        return out

    def to(self, device, **kwargs):
        self.device = torch.device(device)
        return self

    def pin_memory(self):
        self.buf = self.buf.pin_memory()
        return self

    def materialize_host(self, device=None):
        images = torch.stack([s.host() for s in self.samples()])
        return images if device is None else images.to(device, non_blocking=True)

    def materialize(self, device=None):
        """-> images f32 [n,3,H,W] on `device` (default: where `to` sent the batch)"""
        from . import hip
        device = torch.device(self.device if device is None else device)
        res = _planned_on_device(DeferredClsBatch, self, device, hip.host_policy.cls_input_hip,
                                 lambda buf: hip.cls_input(buf, self.desc, self.size, self.mean, self.std))
        return self.materialize_host(device) if res is None else res.images


@register_collate_func
def cls_collate_fn(batch):
    """The collate function of the classification loaders (`evaluation.build_data_loader` gives it to a `config.ImageFolder` that names
    none): planned samples -- (`DeferredClsSample`, label) -- become (`DeferredClsBatch`, LongTensor of labels); anything else goes
    through `torch.utils.data.default_collate`, unchanged."""
    from torch.utils.data import default_collate
    planned = [isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[0], DeferredClsSample) for item in batch]
    if not any(planned):
        return default_collate(batch)
    if not all(planned):
        raise TypeError('a batch mixes planned and transformed samples')
    return DeferredClsBatch([item[0] for item in batch]), default_collate([item[1] for item in batch])


class DeferredDetSample(_PlannedSample):
    """What `coco_data.Compose.plan` hands out in place of the float image: the source bytes as numpy uint8 [h,w,3] and the drawn
    `flip`, so that a data-loader worker converts nothing.  `.shape` is the (3, h, w) of the tensor it stands for; `host()` is that
    tensor: `to_tensor` and the flip."""
    __slots__ = ('image', 'flip')

    def __init__(self, image, flip):
        assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3, 'DeferredDetSample: uint8 [h,w,3] is required'
        self.image, self.flip = image, bool(flip)

    @property
    def shape(self):
        return (3, int(self.image.shape[0]), int(self.image.shape[1]))

    def host(self):
        image = to_tensor(self.image)
        return image.flip(-1) if self.flip else image


class DeferredDetBatch(object):
    """A batch of `DeferredDetSample`s as `coco_collate_fn` packs it: `buf`, one flat CPU uint8 tensor with every image back to back;
    `sizes`, the (h, w) of each -- what a consumer reads in place of `img.shape[-2:]`; `flips`; `offsets`, each image's byte offset in
    `buf`.  `to(device)` only records where the batch is wanted.  `tensors(device)` gives the list of float32 images of the host chain,
    bit for bit the unplanned samples; `transformed(transform, device)` gives the padded batch of a `detection.GeneralizedRCNNTransform`
    and its image sizes by one copy up of `buf` and one sc2_det_input launch, cached per (device, min_size, max_size, mean, std,
    size_divisible): a teacher and a student whose transforms agree share one copy and one launch, and neither may write into the
    tensor; on a device that is not a HIP device it raises.  A slice shares the buffer and its copy on the device.  `release()` drops
    the copies and caches.  `launches` counts the launches of the process (for the tests and the tools)."""
    launches = 0

    def __init__(self, samples, _parts=None):
        if _parts is not None:
            self.buf, self.sizes, self.flips, self.offsets = _parts
        else:
            assert len(samples) >= 1 and all(isinstance(s, DeferredDetSample) for s in samples)
            chunks = [np.ascontiguousarray(s.image).reshape(-1) for s in samples]
            self.buf = torch.from_numpy(np.concatenate(chunks))
            self.sizes = [tuple(s.shape[-2:]) for s in samples]
            self.flips = [s.flip for s in samples]
            self.offsets = [int(v) for v in np.cumsum([0] + [c.size for c in chunks[:-1]])]
        self.device = torch.device('cpu')
        self._on_device = dict()      # device -> the copy of buf there (shared with the slices of this batch)
        self._cache = dict()          # transform parameters -> (padded batch, image sizes)
        self._lists = dict()          # device -> the float32 list of `tensors`

    def __len__(self):
        return len(self.sizes)

    def __getitem__(self, index):
        """a slice: the batch of those samples over the same buffer; an integer: that `DeferredDetSample`, as a view of `buf`"""
        if isinstance(index, slice):
            part = DeferredDetBatch(None, _parts=(self.buf, self.sizes[index], self.flips[index], self.offsets[index]))
            part.device, part._on_device = self.device, self._on_device      # (one buffer: one copy up for all its slices)
            return part
        (h, w), off = self.sizes[index], self.offsets[index]
        return DeferredDetSample(self.buf.numpy()[off:off + 3 * h * w].reshape(h, w, 3), self.flips[index])

    def to(self, device, **kwargs):
        self.device = torch.device(device)
        return self

    def pin_memory(self):
        self.buf = self.buf.pin_memory()
        return self

    def release(self):
        """drops the device copies of `buf` and every cached result (the next `tensors` / `transformed` starts from the host bytes)"""
        self._on_device.clear()
        self._cache.clear()
        self._lists.clear()

    def tensors(self, device=None):
        """the float32 [3,h,w] images of the host chain on `device`, converted once per device: a NEW list of the SAME tensors on every
        call, which a teacher and a student share -- nobody writes into them"""
        device = torch.device(self.device if device is None else device)
        images = self._lists.get(device)
        if images is None:
            host = self._lists.get(torch.device('cpu'))
            if host is None:
                host = self._lists[torch.device('cpu')] = [self[i].host() for i in range(len(self))]
            images = self._lists[device] = host if device.type == 'cpu' else [image.to(device, non_blocking=True) for image in host]
        return list(images)

    def transformed(self, transform, device=None):
        """-> (f32 [n,3,Hp,Wp] on `device`, [(oh, ow)]): what `transform.forward(self.tensors(device))` puts into its ImageList"""
        from . import hip
        device = torch.device(self.device if device is None else device)
        if device.type != 'cuda':
            raise hip.Sc2Error('DeferredDetBatch.transformed: {} is not a HIP device (sc2_det_input has no CPU fallback); call the '
                               'transform itself on the batch, or on `tensors(device)`'.format(device))
        mean, std = tuple(float(v) for v in transform.image_mean), tuple(float(v) for v in transform.image_std)
        key = (device, tuple(transform.min_size), transform.max_size, mean, std, transform.size_divisible)
        hit = self._cache.get(key)
        if hit is not None:
            return hit
        image_sizes = [tuple(int(v) for v in transform.resized_size(h, w)) for h, w in self.sizes]
        stride = float(transform.size_divisible)
        max_h = int(math.ceil(max(s[0] for s in image_sizes) / stride) * stride)
        max_w = int(math.ceil(max(s[1] for s in image_sizes) / stride) * stride)
        rows = [(off, h, w, oh, ow, int(flip)) for off, (h, w), (oh, ow), flip in zip(self.offsets, self.sizes, image_sizes, self.flips)]
        batched = _launch_on_copy(self.buf, device, self._on_device, lambda buf: hip.det_input(      # (every element is written)
            buf, rows, mean, std, torch.empty((len(self), 3, max_h, max_w), dtype=torch.float32, device=device)))
        DeferredDetBatch.launches += -(-len(self) // hip.DET_INPUT_MAX_BATCH)
        self._cache[key] = (batched, image_sizes)
        return batched, image_sizes


def get_transform(name):
    for d in (CODEC_TRANSFORM_MODULE_DICT, MISC_TRANSFORM_MODULE_DICT, TORCHVISION_TRANSFORM_DICT):
        if name in d:
            return d[name]
    return None
