"""The RoI heads' post-processing (`detection.RoIHeads.postprocess_detections`) alone, at the reference's evaluation shape: 6 images x
1 000 proposals x 91 classes, f32 logits and deltas on the device, score threshold 0.05, NMS at 0.5, 100 detections per image --
ms per batch with `host_policy.det_post_hip` on (sc2_det_postprocess: three launches and one read-back) and off (softmax +
decode, then the per-image loop of torch ops around `batched_nms` on sc2_nms), alternating in one process, R rounds of K runs,
host-timed around a synchronise (the loop synchronises per image: device events alone would not see its host side); medians.
Needs no data: seeded random inputs (tests/ref_det_post.py's generator), the logits scaled so that a few hundred candidates per
image pass the threshold (most rows are made background; the counts are printed).

    python tools/det_post_times.py [--rounds R] [--iters K] [--images N] [--thresh T]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sc2bench_amd as S  # noqa: E402,F401
from sc2bench_amd import detection, hip  # noqa: E402
import ref_det_post as RP  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--proposals', type=int, default=1000)
    ap.add_argument('--classes', type=int, default=91)
    ap.add_argument('--thresh', type=float, default=0.05)
    ap.add_argument('--logit-scale', type=float, default=2.2)
    ap.add_argument('--objects', type=float, default=0.08, help='share of the proposals that are not background')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('det_post_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    n, C = args.images, args.classes
    counts, sizes = [args.proposals] * n, [(800, 1216)] * n
    logits, deltas, props = RP.random_case(counts, C, sizes, seed=0, logit_scale=args.logit_scale, clusters=40)
    # as behind a trained head, most proposals are background: all but `--objects` of the rows get a towering background logit
    objects = np.random.RandomState(1).rand(logits.shape[0]) < args.objects
    logits[~objects, 0] += 14.0
    logits, deltas = torch.from_numpy(logits).to(dev), torch.from_numpy(deltas).to(dev)
    proposals = [p.contiguous() for p in torch.from_numpy(props).to(dev).split(counts, 0)]
    heads = detection.RoIHeads(None, None, None, score_thresh=args.thresh, nms_thresh=0.5, detections_per_img=100)
    out = {}

    def post():
        out['det'] = heads.postprocess_detections(logits, deltas, proposals, sizes)
    rows = {True: [], False: []}
    with torch.no_grad():
        for on in (True, False):      # warm-up: code objects, the allocator
            hip.configure(det_post_hip=on)
            post()
            post()
            out[on] = [b.shape[0] for b in out['det'][0]]
        passing = (torch.softmax(logits, -1)[:, 1:] > args.thresh).view(n, -1).sum(1).tolist()
        print('post-processing alone, {} images x {} proposals x {} classes, score threshold {}, device {}'.format(
            n, args.proposals, C, args.thresh, torch.cuda.get_device_name(0)))
        print('candidates above the score threshold per image {}; detections per image: kernel {}, loop {}'.format(passing, out[True], out[False]))
        for _ in range(args.rounds):
            for on in (True, False):
                hip.configure(det_post_hip=on)
                rows[on].append(timed(post, args.iters))
        hip.configure(det_post_hip=True)
        with hip.KernelTimer() as timer:
            post()
            torch.cuda.synchronize()
    hip.configure(det_post_hip=hip.HostPolicy.det_post_hip)
    print('ms per batch, {} alternating rounds of {} runs'.format(args.rounds, args.iters))
    for on, name in ((True, 'det_post_hip on '), (False, 'det_post_hip off')):
        print('{}  median {:8.3f}   rounds {}'.format(name, statistics.median(rows[on]), ' '.join('{:8.3f}'.format(v) for v in rows[on])))
    print('the three launches of one call together (device events): {}'.format(
        ', '.join('{} {:.4f} ms'.format(tag, ms) for tag, (count, ms) in sorted(timer.summary().items()))))


if __name__ == '__main__':
    main()
