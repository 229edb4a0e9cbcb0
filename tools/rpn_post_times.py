"""The RPN's proposal selection alone -- `detection.RegionProposalNetwork.forward` behind its head -- at the reference's evaluation
shape: 6 images, levels 200 x 304, 100 x 152, 50 x 76, 25 x 38 and 13 x 19 with 3 anchors per cell (242 991 anchors per image), f32
head outputs on the device, pre- / post-NMS top-n 1 000 (`--top-n 2000`: the training shape), NMS at 0.7 -- ms per batch with
`host_policy.rpn_post_hip` on (sc2_rpn_proposals: three launches on the head's maps as they stand and one read-back) and off
(concat of the levels, decode of every anchor, one topk per level, three gathers, then the per-image loop of torch ops around
`batched_nms` on sc2_nms), alternating in one process, R rounds of K runs, host-timed around a synchronise (the loop synchronises
per image: device events alone would not see its host side); medians.  Both paths include the anchor generator, timed alone as well.
Needs no data: the head is replaced by seeded maps (tests/ref_rpn_post.py's generator; the spread of the logits and the
proposals kept are printed).

    python tools/rpn_post_times.py [--rounds R] [--iters K] [--images N] [--top-n K]
"""
import argparse
import os
import statistics
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sc2bench_amd as S  # noqa: E402,F401
from sc2bench_amd import detection, hip  # noqa: E402
import ref_rpn_post as RR  # noqa: E402

LEVELS = [(3, 200, 304), (3, 100, 152), (3, 50, 76), (3, 25, 38), (3, 13, 19)]
IMAGE = (800, 1216)


class Computed(torch.nn.Module):
    """stands in for the RPN head: returns the seeded maps"""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return self.out


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
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--top-n', type=int, default=1000)
    ap.add_argument('--logit-scale', type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rpn_post_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    n, top = args.images, args.top_n
    obj, dl, _ = RR.random_case(LEVELS, n, IMAGE, seed=0, logit_scale=args.logit_scale, delta_scale=0.3)
    logits = np.concatenate([o.reshape(n, -1) for o in obj], axis=1)
    head = Computed(([torch.from_numpy(o).to(dev) for o in obj], [torch.from_numpy(d).to(dev) for d in dl]))
    gen = detection.AnchorGenerator(((32,), (64,), (128,), (256,), (512,)), ((0.5, 1.0, 2.0),) * 5)
    rpn = detection.RegionProposalNetwork(gen, head, pre_nms_top_n=dict(training=top, testing=top),
                                          post_nms_top_n=dict(training=top, testing=top), nms_thresh=0.7).eval().to(dev)
    feats = OrderedDict((str(l), torch.zeros(n, 1, s[1], s[2], device=dev)) for l, s in enumerate(LEVELS))
    images = detection.ImageList(torch.zeros(n, 3, IMAGE[0], IMAGE[1], device=dev), [IMAGE] * n)
    out = {}

    def run():
        out['boxes'] = rpn(images, feats)[0]
    rows = {True: [], False: []}
    with torch.no_grad():
        for on in (True, False):      # warm-up: code objects, the allocator
            hip.configure(rpn_post_hip=on)
            run()
            run()
            out[on] = [b.shape[0] for b in out['boxes']]
        print('proposal selection alone, {} images x {} anchors in {} levels, top-n {} / {}, NMS at 0.7, device {}'.format(
            n, logits.shape[1], len(LEVELS), top, top, torch.cuda.get_device_name(0)))
        print('logits: min {:.2f}, median {:.2f}, max {:.2f}, the {}th greatest of level 0 of image 0 {:.2f}'.format(
            logits.min(), float(np.median(logits)), logits.max(), top, float(np.sort(obj[0][0].reshape(-1))[-top])))
        print('proposals kept per image: kernel {}, loop {}'.format(out[True], out[False]))
        for _ in range(args.rounds):
            for on in (True, False):
                hip.configure(rpn_post_hip=on)
                rows[on].append(timed(run, args.iters))
        anchors_ms = timed(lambda: gen(images, list(feats.values())), args.iters)
        hip.configure(rpn_post_hip=True)
        with hip.KernelTimer() as timer:
            run()
            torch.cuda.synchronize()
    hip.configure(rpn_post_hip=hip.HostPolicy.rpn_post_hip)
    print('ms per batch, {} alternating rounds of {} runs'.format(args.rounds, args.iters))
    for on, name in ((True, 'rpn_post_hip on '), (False, 'rpn_post_hip off')):
        print('{}  median {:8.3f}   rounds {}'.format(name, statistics.median(rows[on]), ' '.join('{:8.3f}'.format(v) for v in rows[on])))
    print('of which the anchor generator (both paths): {:.3f} ms'.format(anchors_ms))
    print('the three launches of one call together (device events): {}'.format(
        ', '.join('{} {:.4f} ms'.format(tag, ms) for tag, (count, ms) in sorted(timer.summary().items()) if tag == 'rpn_proposals')))


if __name__ == '__main__':
    main()
