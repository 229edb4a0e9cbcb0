"""`CocoBoxEvaluator.accumulate` on device buffers -- the two kernels -- against the host path of the same module, at a synthetic
COCO val2017 scale: 5 000 images, 80 categories, 100 detections per image, about 7 ground truths per image, fixed seed.  Needs no
data: ground truths are random boxes, a third of the detections are jittered copies of their image's ground truths (so that matches
at every threshold occur), the rest random.

    python tools/coco_eval_times.py [--images N] [--reps R] [--host-reps H] [--forward K] [--out FILE]

Every timing is a host clock around `accumulate()`, which ends in the copy of precision / recall to the host (a synchronise), with
the detections already buffered ON THE DEVICE by `update` in both forms:

    kernels   host_policy.coco_eval_hip = True : torch sorts on the device, sc2_coco_match, sc2_coco_accumulate, one copy back
    host      host_policy.coco_eval_hip = False: the same sorts on the host after the copy, numpy matching and accumulation

plus the HIP-event times of the two launches alone, and a check that both forms return the same bits.

`--forward K` also times K batch-size-1 forwards of the `coco2017` Entropic-Student Faster R-CNN (`dense.faster_rcnn_model`, bf16 body and
pyramid, updated bottleneck, RANDOM weights, a 480 x 640 noise image resized to 800 x 1066 by the model's transform) and prints what
share of `images` such forwards + accumulate() the accumulate() of each form is.  Random weights fix the number of detections that
reach the RoI heads' post-processing only loosely (printed): the share is an order of magnitude, not a figure for a trained model.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc2bench_amd as S  # noqa: E402
from sc2bench_amd import hip  # noqa: E402


def synthetic(images, cats=80, dets=100, gts=7.0, seed=0):
    rng = np.random.RandomState(seed)
    anns, preds = [], {}
    for i in range(images):
        n = rng.poisson(gts)
        xy = rng.rand(n, 2) * 400
        wh = np.exp(rng.randn(n, 2) * 0.8 + 4.0).clip(4, 400)      # sides from a few pixels to the image: all three area ranges
        labels = rng.randint(1, cats + 1, size=n) if rng.rand() > 0.1 else np.full(n, 1 + rng.randint(cats))      # some crowded categories
        for j in range(n):
            anns.append({'id': len(anns) + 1, 'image_id': i, 'category_id': int(labels[j]), 'bbox': [float(v) for v in (*xy[j], *wh[j])],
                         'area': float(wh[j, 0] * wh[j, 1] * rng.uniform(0.4, 0.9)), 'iscrowd': int(rng.rand() < 0.02)})
        box = np.concatenate([rng.rand(dets, 2) * 400, np.exp(rng.randn(dets, 2) * 0.8 + 4.0).clip(4, 400)], 1)
        lab = rng.randint(1, cats + 1, size=dets)
        near = min(n * 4, dets // 3)
        if n:
            src = rng.randint(n, size=near)
            box[:near] = np.concatenate([xy[src], wh[src]], 1) * rng.uniform(0.85, 1.15, size=(near, 4))
            lab[:near] = labels[src]
        box[:, 2:] += box[:, :2]
        preds[i] = {'boxes': torch.from_numpy(box.astype(np.float32)), 'scores': torch.from_numpy(rng.rand(dets).astype(np.float32)),
                    'labels': torch.from_numpy(lab.astype(np.int64))}
    gt = {'images': [{'id': i} for i in range(images)], 'annotations': anns, 'categories': [{'id': c} for c in range(1, cats + 1)]}
    return gt, preds


def forward_ms(dev, iters):
    """-> (ms per bs-1 forward, detections of the last one)"""
    from sc2bench_amd import dense
    torch.manual_seed(0)
    backbone = {'key': 'splittable_resnet',
                'kwargs': {'num_classes': 1000, 'pretrained': False, 'resnet_name': 'resnet50', 'pre_transform': None, 'skips_avgpool': True,
                           'skips_fc': True, 'bottleneck_config': {'key': 'FPBasedResNetBottleneck',
                                                                   'kwargs': {'num_bottleneck_channels': 24, 'num_target_channels': 256}}}}
    model = dense.faster_rcnn_model(backbone, pretrained=False, num_classes=91, backbone_fpn_kwargs={
        'return_layer_dict': {'bottleneck_layer': '1', 'layer2': '2', 'layer3': '3', 'layer4': '4'},
        'in_channels_list': [256, 512, 1024, 2048], 'out_channels': 256, 'analyzable_layer_key': 'bottleneck_layer'})
    model.eval().to(dev)
    model.update()
    model.backbone.body.set_compute_dtype('bf16')
    model.backbone.fpn.to(torch.bfloat16)
    image = torch.rand(3, 480, 640, generator=torch.Generator().manual_seed(0)).to(dev)
    with torch.inference_mode():
        for _ in range(3):
            out = model([image])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = model([image])
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters, int(out[0]['boxes'].shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--forward', type=int, default=0)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    gt, preds = synthetic(args.images)
    lines = ['coco_eval_times: {} images, 80 categories, {} detections, {} ground truths, seed 0, {}'.format(
        args.images, sum(len(p['scores']) for p in preds.values()), len(gt['annotations']), torch.cuda.get_device_name(0))]
    ev = S.CocoBoxEvaluator(gt)
    for i in range(0, args.images, 8):      # as the evaluation loop does: a few images per update, tensors on the device
        ev.update({k: {n: t.to(dev) for n, t in preds[k].items()} for k in range(i, min(i + 8, args.images))})
    torch.cuda.synchronize()

    def run(on):
        hip.configure(coco_eval_hip=on)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.accumulate()
        return time.perf_counter() - t0

    run(True)      # warm-up: code objects, allocator
    be = ev.coco_eval['bbox']
    assert be.path == 'hip'
    kernels = [run(True) for _ in range(args.reps)]
    p_hip, r_hip = be.eval['precision'].copy(), be.eval['recall'].copy()
    with hip.KernelTimer() as timer:
        run(True)
    torch.cuda.synchronize()
    launches = timer.summary()
    host = []
    for _ in range(args.host_reps):
        host.append(run(False))
        print('host path: {:.1f} s'.format(host[-1]), flush=True)
    assert be.path == 'host'
    same = np.array_equal(be.eval['precision'], p_hip) and np.array_equal(be.eval['recall'], r_hip)
    hip.configure(coco_eval_hip=True)
    ev.summarize()
    med_k, med_h = statistics.median(kernels), statistics.median(host)
    lines.append('accumulate(), kernels : median {:.1f} ms of {} runs (min {:.1f}, max {:.1f})'.format(
        1e3 * med_k, len(kernels), 1e3 * min(kernels), 1e3 * max(kernels)))
    for tag in ('coco_match', 'coco_accumulate'):
        lines.append('  launch {:<16}: {:.3f} ms (HIP events, one run)'.format(tag, launches[tag][1]))
    lines.append('accumulate(), host    : median {:.1f} ms of {} run(s)'.format(1e3 * med_h, len(host)))
    lines.append('host / kernels        : {:.1f} x'.format(med_h / med_k))
    lines.append('same precision / recall bits in both forms: {}'.format(same))
    lines.append('AP {:.6f}  AP50 {:.6f}  AR100 {:.6f}'.format(be.stats[0], be.stats[1], be.stats[8]))
    if args.forward:
        fwd, n_out = forward_ms(dev, args.forward)
        total = 1e-3 * fwd * args.images
        lines.append('bs-1 forward (random weights, 480 x 640 -> 800 x 1066, {} detections out): {:.1f} ms, x {} images = {:.1f} s'.format(
            n_out, fwd, args.images, total))
        lines.append('accumulate() share of forwards + accumulate(): kernels {:.2%}, host {:.2%}'.format(med_k / (total + med_k), med_h / (total + med_h)))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    assert same, 'the two forms differ'


if __name__ == '__main__':
    main()
