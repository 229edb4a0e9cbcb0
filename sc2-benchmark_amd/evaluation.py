"""Evaluation loop of the image-classification task (script/task/image_classification.py:106-145) and the
`-test_only` entry for the BASELINE plumbing configs:

    python -m sc2bench_amd.evaluation --config <yaml> [--device cpu|cuda] [--json '{...}'] [--max_samples 100]

It builds `models.model` (or `models.student_model`) from the reference's YAML file unchanged, loads `test.test_data_loader`
(dataset, sampler, batch size, `collate_fn`), runs the model in eval mode under `torch.inference_mode()`, reports top-1 /
top-5 accuracy (mIoU for a segmentation model, COCO box AP for a Faster R-CNN) and lets every analyzer summarise (data size in KB, as the reference logs it).  Metric totals and counts are
summed over ranks when a process group is up (`MetricLogger.synchronize_between_processes`: SURVEY.md C5).
"""
import argparse
import json
import logging
import time

import torch

from . import config as C
from .analysis import AnalyzableModule
from .dataparallel import all_reduce_sum_scalars

logger = logging.getLogger(__name__)


def compute_accuracy(outputs, targets, topk=(1,)):
    """-> [accuracy@k in percent] (image_classification.py:91-103)."""
    with torch.no_grad():
        maxk = max(topk)
        batch_size = targets.size(0)
        _, preds = outputs.topk(maxk, 1, True, True)
        corrects = preds.t().eq(targets[None])
        return [corrects[:k].flatten().sum(dtype=torch.float32) * (100.0 / batch_size) for k in topk]


class Meter(object):
    def __init__(self):
        self.total, self.count = 0.0, 0

    def update(self, value, n=1):
        self.total += float(value) * n
        self.count += n

    @property
    def global_avg(self):
        return self.total / max(1, self.count)


def _pipelined(model, data_loader, device, pipeline):
    """True if evaluate() should run the batches through `pipeline.StagePipeline`: an updated bottleneck model on a HIP device,
    batches of more than one image (the reference measures data size at batch size 1, README.md:100-108: those runs keep the
    per-batch forward, bytes objects and analyzers), and no analyzer that wants the compressed object of every batch."""
    if pipeline is False or device.type != 'cuda':
        return False
    from .pipeline import supports_stages
    if not supports_stages(model):
        return False
    if getattr(model, 'analyzes_after_compress', False) and getattr(model, 'analyzers', None):
        return False
    return pipeline is True or (getattr(data_loader, 'batch_size', None) or 1) > 1


def _evaluate_pipelined(model, data_loader, device, max_samples, pipeline_kwargs):
    """The loop of evaluate() on the stage pipeline: front stages run ahead, the range coder of several batches shares a
    launch on its own HIP stream, top-1 / top-5 hits are counted on the device behind each back stage -- the host reads
    two numbers at the end instead of two per batch.  -> (correct@1, correct@5, samples) as floats."""
    from .pipeline import StagePipeline
    from .transforms import DeferredClsBatch
    pipe = StagePipeline(model, device, **(pipeline_kwargs or {}))
    # one row of hit counters per back stream: back stage j runs on back stream j % len(back_streams), and two streams adding
    # into the same two addresses would race
    n_back = len(pipe.back_streams)
    hits = torch.zeros(n_back, 2, dtype=torch.float64, device=device)
    targets = {}
    seen = [0]

    def batches():
        for i, (image, target) in enumerate(data_loader):
            if max_samples is not None and seen[0] >= max_samples:
                return
            targets[i] = target.to(device, non_blocking=True)
            seen[0] += len(image)
            # (a planned batch -- transforms.DeferredClsBatch -- is finished here, on the caller's stream like the copy it replaces: the
            #  front stage's wait on that stream orders its launch before the encoder)
            yield image.materialize(device) if isinstance(image, DeferredClsBatch) else image.to(device, non_blocking=True)

    def on_output(step, output, nbytes, status):
        # called inside the back stream's context.  The labels were copied on the caller's stream (ordered before this point
        # through the front stage's wait on it -> coder event -> back stream), but the caching allocator only knows the stream a
        # block was ALLOCATED on: without record_stream it would hand the block to a later batch's `target.to(device)` as soon as
        # `target` dies here, while the back stream's eq / topk kernels -- queued milliseconds behind the coder -- still read it
        target = targets.pop(step)
        bs = torch.cuda.current_stream(device)
        target.record_stream(bs)
        row = hits[step % n_back]
        _, preds = output.float().topk(5, 1, True, True)
        corrects = preds.t().eq(target[None])
        row[0] += corrects[:1].sum(dtype=torch.float64)
        row[1] += corrects[:5].sum(dtype=torch.float64)

    record = {}
    pipe.run(batches(), on_output=on_output, record=record)
    pipe.synchronize()
    from .entropy import _raise_on_status
    for st in record['statuses']:       # every coder launch of the run, read once at the end
        _raise_on_status(st, 'evaluate (stage pipeline)')
    h = hits.sum(0).cpu()
    return float(h[0]), float(h[1]), seen[0]


@torch.inference_mode()
def evaluate(model, data_loader, device, max_samples=None, log_freq=1000, title=None, pipeline=None, pipeline_kwargs=None):
    """-> {'acc1', 'acc5', 'samples', 'seconds', 'analysis': [summaries]}.  `pipeline`: None = the stage pipeline
    (sc2bench_amd/pipeline.py) when the model is an updated bottleneck model on a HIP device and the loader's batches hold more
    than one image; True / False force it on / off."""
    model = model.to(device) if device.type == 'cuda' else model
    if hasattr(model, 'use_cpu4compression') and device.type != 'cuda':
        model.use_cpu4compression()
    if title is not None:
        logger.info(title)
    model.eval()
    analyzable = isinstance(model, AnalyzableModule)
    if analyzable:
        model.activate_analysis()
    acc1, acc5 = Meter(), Meter()
    t0 = time.perf_counter()
    seen = 0
    pipelined = _pipelined(model, data_loader, device, pipeline)
    if pipelined:
        c1, c5, seen = _evaluate_pipelined(model, data_loader, device, max_samples, pipeline_kwargs)
        acc1.total, acc1.count = 100.0 * c1, seen       # (Meter: sum of percent x batch size, and the sample count)
        acc5.total, acc5.count = 100.0 * c5, seen
    from .transforms import DeferredClsBatch
    for i, (image, target) in enumerate(() if pipelined else data_loader):
        if isinstance(image, DeferredClsBatch):     # a planned ImageNet batch: crop, resize, ToTensor and Normalize run here, on `device`
            image = image.materialize(device)
        if isinstance(image, torch.Tensor):
            image = image.to(device, non_blocking=True)
        if isinstance(target, torch.Tensor):
            target = target.to(device, non_blocking=True)
        output = model(image)
        a1, a5 = compute_accuracy(output.float(), target.to(output.device), topk=(1, 5))
        batch_size = len(image)
        acc1.update(a1.item(), n=batch_size)
        acc5.update(a5.item(), n=batch_size)
        seen += batch_size
        if log_freq and (i + 1) % log_freq == 0:
            logger.info('Test: [{}] acc1 {:.3f} acc5 {:.3f}'.format(i + 1, acc1.global_avg, acc5.global_avg))
        if max_samples is not None and seen >= max_samples:
            break
    # totals and counts are summed over ranks and divided afterwards (MetricLogger.synchronize_between_processes), on the
    # backend's device: an RCCL-only process group cannot reduce a host tensor
    t1, c1, t5, c5, seen_all = all_reduce_sum_scalars([acc1.total, acc1.count, acc5.total, acc5.count, seen])
    top1, top5 = t1 / max(1.0, c1), t5 / max(1.0, c5)
    logger.info(' * Acc@1 {:.4f}\tAcc@5 {:.4f}\n'.format(top1, top5))
    analysis = []
    if analyzable and model.activated_analysis:
        model.summarize()
        analysis = [a.summary() for a in model.analyzers if hasattr(a, 'summary') and getattr(a, 'file_size_list', None)]
    return {'acc1': top1, 'acc5': top5, 'samples': seen, 'samples_all_ranks': int(seen_all), 'seconds': time.perf_counter() - t0, 'analysis': analysis,
            'pipeline': 'stage pipeline (sc2bench_amd/pipeline.py)' if pipelined else 'none: module forward per batch'}


def evaluate_segmentation(model, data_loader, device, num_classes, max_samples=None, log_freq=1000, title=None):
    """The evaluation loop of the semantic-segmentation task (script/task/semantic_segmentation.py:95-134): eval mode, analysis
    on, every batch's labels counted into a `SegEvaluator`, the matrix summed over ranks, the analyzers summarised.
    A model with `predict` (dense.BaseSegmentationModel) labels and counts from its LOW-resolution logits -- on a HIP device
    one `sc2_seg_predict` launch per batch, no resized logits; any other model runs `model(images)['out'].argmax(1)` into
    `SegEvaluator.update` as the reference does.
    -> {'miou', 'acc_global', 'iou', 'acc', 'samples', 'seconds', 'analysis', 'evaluator'}."""
    from .dense import SegEvaluator
    # moved BEFORE inference mode is entered: tensors created under it (a model built on the host and copied here) do not track the
    # version counter that the coder's table caches key on
    model = model.to(device) if device.type == 'cuda' else model
    with torch.inference_mode():
        return _evaluate_segmentation(model, data_loader, device, num_classes, SegEvaluator(num_classes), max_samples, log_freq, title)


def _evaluate_segmentation(model, data_loader, device, num_classes, evaluator, max_samples, log_freq, title):
    if hasattr(model, 'use_cpu4compression') and device.type != 'cuda':
        model.use_cpu4compression()
    if title is not None:
        logger.info(title)
    model.eval()
    analyzable = isinstance(model, AnalyzableModule)
    if analyzable:
        model.activate_analysis()
    fused = callable(getattr(model, 'predict', None))
    t0 = time.perf_counter()
    seen = 0
    from .transforms import DeferredSegBatch
    for i, batch in enumerate(data_loader):
        if isinstance(batch, DeferredSegBatch):     # a planned PASCAL batch: resize, ToTensor and Normalize run here, on `device`
            images, targets = batch.materialize(device)
        else:
            images, targets = batch[0], batch[1]
        if isinstance(images, torch.Tensor):
            images = images.to(device, non_blocking=True)
        if isinstance(targets, torch.Tensor):
            targets = targets.to(device, non_blocking=True)
        if fused:
            if evaluator.mat is None:
                evaluator.mat = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=targets.device)
            model.predict(images, targets, evaluator.mat)
        else:
            evaluator.update(targets.flatten(), model(images)['out'].argmax(1).flatten())
        seen += len(images)
        if log_freq and (i + 1) % log_freq == 0:
            logger.info('Test: [{}] {} samples'.format(i + 1, seen))
        if max_samples is not None and seen >= max_samples:
            break
    evaluator.reduce_from_all_processes()
    logger.info(str(evaluator))
    acc_global, acc, iou = evaluator.compute()
    analysis = []
    if analyzable and model.activated_analysis:
        model.summarize()
        analysis = [a.summary() for a in model.analyzers if hasattr(a, 'summary') and getattr(a, 'file_size_list', None)]
    return {'miou': iou.mean().item(), 'acc_global': acc_global.item(), 'iou': iou.tolist(), 'acc': acc.tolist(), 'samples': seen,
            'seconds': time.perf_counter() - t0, 'analysis': analysis, 'evaluator': evaluator}


def evaluate_detection(model, data_loader, device, gt=None, max_samples=None, log_freq=1000, title=None, iou_types=('bbox',)):
    """The evaluation loop of the object-detection task (script/task/object_detection.py:117-175): eval mode, analysis on, images as a
    list on the device, the model's outputs LEFT on the device and buffered by a `CocoBoxEvaluator` under the image ids read from the
    host-side targets; detections of all ranks are gathered, box AP is accumulated (coco_eval.py: two launches on a HIP device), the
    twelve lines are logged and the analyzers summarised.  `gt`: anything `CocoBoxEvaluator` takes; None = `coco_gt_from_dataset` of the
    loader's dataset.  -> {'map', 'stats', 'summary' (the printed lines), 'samples', 'seconds', 'analysis', 'evaluator'}."""
    from .coco_eval import CocoBoxEvaluator, coco_gt_from_dataset
    evaluator = CocoBoxEvaluator(coco_gt_from_dataset(data_loader.dataset) if gt is None else gt, iou_types)
    model = model.to(device) if device.type == 'cuda' else model
    with torch.inference_mode():
        return _evaluate_detection(model, data_loader, device, evaluator, max_samples, log_freq, title)


def _evaluate_detection(model, data_loader, device, evaluator, max_samples, log_freq, title):
    import contextlib
    import io
    if hasattr(model, 'use_cpu4compression') and device.type != 'cuda':
        model.use_cpu4compression()
    if title is not None:
        logger.info(title)
    model.eval()
    analyzable = isinstance(model, AnalyzableModule)
    if analyzable:
        model.activate_analysis()
    t0 = time.perf_counter()
    seen = 0
    from .transforms import DeferredDetBatch
    for i, (images, targets) in enumerate(data_loader):
        if max_samples is not None and seen + len(images) > max_samples:
            images, targets = images[:max_samples - seen], targets[:max_samples - seen]
        image_ids = [int(t['image_id']) for t in targets]      # host-side targets: read before anything is moved
        if isinstance(images, DeferredDetBatch):      # a planned COCO batch: the detector's transform finishes it, on `device`
            images = images.to(device)
        else:
            images = [image.to(device, non_blocking=True) for image in images]
        outputs = model(images)
        evaluator.update({image_id: output for image_id, output in zip(image_ids, outputs)})
        seen += len(images)
        if log_freq and (i + 1) % log_freq == 0:
            logger.info('Test: [{}] {} samples'.format(i + 1, seen))
        if max_samples is not None and seen >= max_samples:
            break
    evaluator.synchronize_between_processes()
    evaluator.accumulate()
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        evaluator.summarize()
    logger.info(printed.getvalue())
    analysis = []
    if analyzable and model.activated_analysis:
        model.summarize()
        # (an InputCompressionDetectionModel's analyzers are those of its transform)
        transform = getattr(getattr(model, 'detection_model', None), 'transform', None)
        analyzers = list(model.analyzers) + list(transform.analyzers if isinstance(transform, AnalyzableModule) else ())
        analysis = [a.summary() for a in analyzers if hasattr(a, 'summary') and getattr(a, 'file_size_list', None)]
    stats = evaluator.coco_eval[evaluator.iou_types[0]].stats
    return {'map': float(stats[0]), 'stats': stats.tolist(), 'summary': printed.getvalue(), 'samples': seen, 'seconds': time.perf_counter() - t0,
            'analysis': analysis, 'evaluator': evaluator}


def build_data_loader(dataset_dict, loader_config):
    """`test.test_data_loader` or `train_data_loader` block -> DataLoader (dataset by id, sampler class, kwargs, `collate_fn` by name).
    `batch_sampler: {key, kwargs}`: the class of that name in `coco_data.BATCH_SAMPLER_DICT`, built as `cls(sampler, **kwargs)`; the
    DataLoader then gets no `batch_size` (torchdistill's behaviour, [recalled])."""
    from .transforms import COLLATE_FUNC_DICT
    dataset = dataset_dict[loader_config['dataset_id']]
    if isinstance(dataset, dict) and 'coco_gt' in dataset:      # `--json`: a COCO dictionary (or its path) in place of the dataset
        from .coco_eval import CocoDictDetection
        dataset = CocoDictDetection(dataset['coco_gt'], seed=dataset.get('seed', 0))
    kwargs = dict(loader_config.get('kwargs') or {})
    sampler_cfg = loader_config.get('sampler') or {}
    sampler_cls = sampler_cfg.get('class_or_func')
    sampler = None
    if sampler_cls is not None and not isinstance(sampler_cls, C.Placeholder):
        sampler = sampler_cls(dataset, **(sampler_cfg.get('kwargs') or {}))
    collate = COLLATE_FUNC_DICT.get(loader_config.get('collate_fn'))      # default_collate_w_pil, pascal_seg_collate_fn, pascal_seg_eval_collate_fn
    if loader_config.get('collate_fn') is None and isinstance(dataset, C.ImageFolder):
        collate = COLLATE_FUNC_DICT['cls_collate_fn']      # default_collate, but for the samples an ImageFolder plans ...
        dataset.plan_samples = True                         # ... which it does for this collate function only
    batch_sampler_cfg = loader_config.get('batch_sampler')
    if batch_sampler_cfg is not None:
        from .coco_data import BATCH_SAMPLER_DICT
        key = batch_sampler_cfg.get('key') if isinstance(batch_sampler_cfg, dict) else None
        if key not in BATCH_SAMPLER_DICT:
            raise KeyError('batch_sampler `{}` is not available (have {})'.format(key, sorted(BATCH_SAMPLER_DICT)))
        sampler_kwargs = dict(batch_sampler_cfg.get('kwargs') or {})
        unresolved = [k for k, v in sampler_kwargs.items() if isinstance(v, C.Placeholder)]
        if unresolved:
            raise ValueError('batch_sampler `{}`: kwargs {} are unresolved (a dataset that is not available leaves '
                             '`custom.sampler.create_aspect_ratio_groups` unresolved)'.format(key, unresolved))
        if sampler is None:
            sampler = torch.utils.data.SequentialSampler(dataset)
        batch_sampler = BATCH_SAMPLER_DICT[key](sampler, **sampler_kwargs)
        kwargs.pop('batch_size', None)
        return torch.utils.data.DataLoader(dataset, batch_sampler=batch_sampler, collate_fn=collate, **kwargs)
    kwargs.setdefault('batch_size', 1)
    return torch.utils.data.DataLoader(dataset, sampler=sampler, collate_fn=collate, **kwargs)


def _classifier_classes(model):
    """output channels of a segmentation model's classifier: its last convolution"""
    convs = [m for m in model.classifier.modules() if isinstance(m, torch.nn.Conv2d)]
    if not convs:
        raise ValueError('cannot tell the number of classes of {}: set test.num_classes'.format(type(model.classifier).__name__))
    return convs[-1].out_channels


def test_only(config, device, max_samples=None, num_workers=None):
    """The `-test_only` branch of main() (image_classification.py:236-250) for a config dict: -> evaluate()'s result."""
    C.import_dependencies(config.get('dependencies'))
    models = config['models']
    model_config = models['student_model'] if 'student_model' in models else models['model']
    model = C.build_model(model_config, device)
    from .ckpt import load_ckpt
    if model_config.get('dst_ckpt') is not None or model_config.get('src_ckpt') is not None:
        load_ckpt(model_config.get('dst_ckpt') or model_config.get('src_ckpt'), model=model, strict=False)
    if hasattr(model, 'update') and not isinstance(model, torch.nn.parallel.DistributedDataParallel):
        from .backbone import check_if_updatable
        if check_if_updatable(model):
            model.update()
    loader_config = dict(config['test']['test_data_loader'])
    if num_workers is not None:
        loader_config['kwargs'] = dict(loader_config.get('kwargs') or {}, num_workers=num_workers)
    loader = build_data_loader(config['datasets'], loader_config)
    from .dense import BaseSegmentationModel
    if isinstance(model, BaseSegmentationModel):
        # the reference's segmentation main() updates an updatable model before its test-only evaluation (semantic_segmentation.py:239)
        body = model._body()
        if not model.bottleneck_updated and hasattr(body, 'check_if_updatable') and body.check_if_updatable():
            model.update()
        num_classes = ((model_config.get('kwargs') or {}).get('num_classes') or config['test'].get('num_classes') or
                       _classifier_classes(model))
        return evaluate_segmentation(model, loader, device, num_classes, max_samples=max_samples, title='[Student/model]')
    from .wrapper import CodecInputCompressionSegmentationModel, InputCompressionDetectionModel
    if isinstance(model, CodecInputCompressionSegmentationModel):      # the codec baseline: the class count is the inner model's
        inner = model.segmentation_model
        num_classes = (((model_config.get('segmentation_model') or {}).get('kwargs') or {}).get('num_classes') or
                       config['test'].get('num_classes') or _classifier_classes(inner))
        return evaluate_segmentation(model, loader, device, num_classes, max_samples=max_samples, title='[Student/model]')
    if isinstance(model, InputCompressionDetectionModel):
        return evaluate_detection(model, loader, device, max_samples=max_samples, title='[Student/model]')
    from .dense import BaseRCNN
    from .detection import FasterRCNN
    if isinstance(model, (FasterRCNN, BaseRCNN)):
        body = model._body() if isinstance(model, BaseRCNN) else None
        if body is not None and not model.bottleneck_updated and hasattr(body, 'check_if_updatable') and body.check_if_updatable():
            model.update()
        return evaluate_detection(model, loader, device, max_samples=max_samples, title='[Student/model]')
    return evaluate(model, loader, device, max_samples=max_samples, title='[Student/model]')


def main(argv=None):
    ap = argparse.ArgumentParser(description='test-only evaluation of a reference config on this build')
    ap.add_argument('--config', required=True)
    ap.add_argument('--json', help='json string to overwrite config')
    ap.add_argument('--device', default='cuda' if torch.cuda.is_available() else 'cpu')
    ap.add_argument('--max_samples', type=int)
    ap.add_argument('--num_workers', type=int)
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    config = C.load_yaml_file(args.config)
    if args.json:
        C.overwrite_config(config, json.loads(args.json))
    result = test_only(config, torch.device(args.device), args.max_samples, args.num_workers)
    if 'summary' in result:
        print(result['summary'], end='')      # a detection run: the twelve lines of COCOeval's summary
    print(json.dumps({k: v for k, v in result.items() if k not in ('evaluator', 'summary')}))      # (the evaluator object of a segmentation / detection run stays in the returned dict)
    return result


if __name__ == '__main__':
    main()
