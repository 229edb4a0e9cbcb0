"""The detection tail (detection.FasterRCNN's RPN and RoI heads) on random f32 pyramid features at the 800 x 1216, 6-image shape
of BASELINE config 4: ms per batch of each stage --

    rpn head         3x3 conv + ReLU, objectness and box-delta 1x1 convs on the five maps (torch ops)
    proposal filter  anchors, decode, top-k, clip, batched NMS by level at 0.7 (sc2_nms), first 1000
    roi align        MultiScaleRoIAlign 7 x 7, sampling ratio 2 (sc2_roi_align)
    box head         TwoMLPHead + FastRCNNPredictor (torch ops)
    post-processing  softmax, per-class decode, clip, score / size filters, batched NMS by label at 0.5 (sc2_nms), first 100

with `host_policy.nms_hip` / `host_policy.roi_align_hip` on (the kernels) and off (the torch-op restatement), alternating, R
rounds (default 3), device events around K runs of a stage.  Needs no data: random features, random weights (the class
scores are spread so that a few thousand boxes per image pass the 0.05 score threshold; the counts are printed).

    python tools/det_tail_times.py [--rounds R] [--images N]
"""
import argparse
import collections
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc2bench_amd as S  # noqa: E402,F401
from sc2bench_amd import detection, hip  # noqa: E402

STAGES = ('rpn head', 'proposal filter', 'roi align', 'box head', 'post-processing')


class Pyramid(torch.nn.Module):
    out_channels = 256


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--iters', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('det_tail_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = detection.FasterRCNN(Pyramid(), 91).eval()
    with torch.no_grad():
        model.roi_heads.box_predictor.cls_score.weight.mul_(30.0)
        model.roi_heads.box_predictor.bbox_pred.weight.mul_(8.0)
    model.to(dev)
    H, W, n = 800, 1216, args.images
    g = torch.Generator().manual_seed(0)
    feats = collections.OrderedDict((name, torch.randn(n, 256, -(-H // s), -(-W // s), generator=g).to(dev))
                                    for name, s in zip(['1', '2', '3', '4', 'pool'], [4, 8, 16, 32, 64]))
    images = detection.ImageList(torch.zeros(n, 3, H, W, device=dev), [(H, W)] * n)
    rpn, rh = model.rpn, model.roi_heads
    state = {}

    def rpn_head():
        state['head'] = rpn.head(list(feats.values()))

    def proposal_filter():
        objectness, deltas = state['head']
        fl = list(feats.values())
        anchors = rpn.anchor_generator(images, fl)
        per_level = [o[0].numel() for o in objectness]
        objectness, deltas = detection.concat_box_prediction_layers(objectness, deltas)
        proposals = rpn.box_coder.decode(deltas.float(), anchors).view(len(anchors), -1, 4)
        state['proposals'] = rpn.filter_proposals(proposals, objectness.float(), images.image_sizes, per_level)[0]

    def roi_align():
        state['pooled'] = rh.box_roi_pool(feats, state['proposals'], images.image_sizes)

    def box_head():
        state['pred'] = rh.box_predictor(rh.box_head(state['pooled']))

    def post():
        logits, reg = state['pred']
        state['det'] = rh.postprocess_detections(logits.float(), reg.float(), state['proposals'], images.image_sizes)
    fns = collections.OrderedDict(zip(STAGES, (rpn_head, proposal_filter, roi_align, box_head, post)))
    settings = collections.OrderedDict((('kernels', (True, True)), ('nms off', (False, True)), ('roi_align off', (True, False))))
    rows = {(s, st): [] for s in settings for st in STAGES}
    with torch.no_grad():
        for fn in fns.values():      # warm-up: code objects, the library's algorithm choices
            fn()
            fn()
        scores = torch.softmax(state['pred'][0].float(), -1)[:, 1:]
        print('detection tail, {} images of {} x {}, f32 pyramid features, device {}'.format(n, H, W, torch.cuda.get_device_name(0)))
        print('proposals per image {}; boxes above the 0.05 score threshold per image about {}; detections per image {}'.format(
            [p.shape[0] for p in state['proposals']], int((scores > 0.05).sum().item()) // n, [b.shape[0] for b in state['det'][0]]))
        for _ in range(args.rounds):
            for name, (nms_on, roi_on) in settings.items():
                hip.configure(nms_hip=nms_on, roi_align_hip=roi_on)
                for stage, fn in fns.items():
                    rows[(name, stage)].append(timed(fn, args.iters))
        hip.configure(nms_hip=True, roi_align_hip=True)
    print('ms per batch, {} alternating rounds of {} runs'.format(args.rounds, args.iters))
    for stage in STAGES:
        print('{:<16}'.format(stage) + '   '.join('{} {}'.format(name, ' '.join('{:9.3f}'.format(v) for v in rows[(name, stage)]))
                                                  for name in settings))
    with torch.no_grad(), hip.KernelTimer() as timer:
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
    print('the kernels of one pass (launches, mean ms):')
    for tag, (count, ms) in sorted(timer.summary().items()):
        print('  {:<12} {:4d} {:9.4f}'.format(tag, count, ms))


if __name__ == '__main__':
    main()
