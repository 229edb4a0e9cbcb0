"""The segmentation evaluation tail alone -- low-resolution logits -> labels at the input's size -> confusion matrix -- at the
shape of BASELINE config 5: 16 x 21 x 65 x 65 -> 513 x 513, bf16 logits as `HipDenseHead` returns them (the permuted view of NHWC
memory with channel pitch 24) and int64 targets.  Four forms, alternating, R repetitions in one process, HIP events around K runs:

    torch bf16    F.interpolate(bf16 logits) -> argmax(1) -> SegEvaluator.update       (what model(x)['out'] fed before `predict`)
    torch f32     `host_policy.seg_predict_hip = False`: interpolate(logits.float()) -> argmax -> bincount (dense.seg_labels)
    kernel        `host_policy.seg_predict_hip = True`: one sc2_seg_predict launch (labels stored, matrix added to)
    kernel, no labels   SegEvaluator.update_logits: the same launch without the label store

and the medians with their ratios.  Needs no data: random logits, random targets (every class and the ignore label 255).

    python tools/seg_tail_times.py [--reps R] [--iters K] [--images N] [--forms]

`--forms` adds the kernel alone in the forms that tell what it spends its time on: labels only, counting with random / constant /
all-ignored targets (441 / 21 / 0 non-zero bins per workgroup to flush), and NCHW bf16 / f32 logits (the strided path).
"""
import argparse
import collections
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc2bench_amd as S  # noqa: E402,F401
from sc2bench_amd import dense, hip  # noqa: E402


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def kernel_forms(logits, targets, size, reps, iters):
    c = logits.shape[1]
    mat = torch.zeros(c, c, dtype=torch.int64, device=logits.device)
    nchw, f32 = logits.contiguous(), logits.float().contiguous()
    constant, ignored = torch.full_like(targets, 3), torch.full_like(targets, 255)
    forms = collections.OrderedDict((
        ('nhwc, labels only', lambda: hip.seg_predict(logits, size)),
        ('nhwc, random targets, labels', lambda: hip.seg_predict(logits, size, targets, mat)),
        ('nhwc, random targets, no labels', lambda: hip.seg_predict(logits, size, targets, mat, want_labels=False)),
        ('nhwc, constant targets, no labels', lambda: hip.seg_predict(logits, size, constant, mat, want_labels=False)),
        ('nhwc, ignored targets, no labels', lambda: hip.seg_predict(logits, size, ignored, mat, want_labels=False)),
        ('nchw bf16, labels only', lambda: hip.seg_predict(nchw, size)),
        ('nchw f32, labels only', lambda: hip.seg_predict(f32, size))))
    for fn in forms.values():
        fn()
    print('the kernel alone, ms per launch, {} repetitions of {} runs'.format(reps, iters))
    for name, fn in forms.items():
        ts = [timed(fn, iters) for _ in range(reps)]
        print('{:<36} median {:8.4f}   all {}'.format(name, statistics.median(ts), ' '.join('{:.4f}'.format(v) for v in ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--forms', action='store_true')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--images', type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('seg_tail_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    n, c, h, w, H, W = args.images, 21, 65, 65, 513, 513
    g = torch.Generator().manual_seed(0)
    nhwc = torch.zeros(n, h, w, 24, dtype=torch.bfloat16)
    nhwc[..., :c] = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16)
    logits = nhwc.to(dev)[..., :c].permute(0, 3, 1, 2)
    targets = torch.randint(0, c + 1, (n, H, W), generator=g)
    targets[targets == c] = 255
    targets = targets.to(dev)
    ev = dense.SegEvaluator(c)
    ev.mat = torch.zeros(c, c, dtype=torch.int64, device=dev)

    def torch_bf16():
        labels = F.interpolate(logits, size=(H, W), mode='bilinear', align_corners=False).argmax(1)
        ev.update(targets.flatten(), labels.flatten())

    def switch(on):
        def run():
            hip.configure(seg_predict_hip=on)
            dense.seg_labels(logits, (H, W), targets, ev.mat)
        return run

    def no_labels():
        hip.configure(seg_predict_hip=True)
        ev.update_logits(targets, logits)
    forms = collections.OrderedDict((('torch bf16', torch_bf16), ('torch f32', switch(False)), ('kernel', switch(True)),
                                     ('kernel, no labels', no_labels)))
    rows = {name: [] for name in forms}
    with torch.no_grad():
        for fn in forms.values():      # warm-up: code objects, the allocator's blocks
            fn()
            fn()
        for _ in range(args.reps):
            for name, fn in forms.items():
                rows[name].append(timed(fn, args.iters))
        # what the forms compute: the same matrix from the two f32 forms up to labels at near-ties, the bf16 form's flips
        mats = {}
        for name, fn in forms.items():
            ev.mat.zero_()
            fn()
            mats[name] = ev.mat.clone()
        hip.configure(seg_predict_hip=True)
        up16 = F.interpolate(logits, size=(H, W), mode='bilinear', align_corners=False).argmax(1)
        up32 = F.interpolate(logits.float(), size=(H, W), mode='bilinear', align_corners=False).argmax(1)
        fused = hip.seg_predict(logits, (H, W))
        total = fused.numel()
        print('segmentation tail, {} x {} x {} x {} -> {} x {}, bf16 NHWC logits (pitch 24), device {}'.format(
            n, c, h, w, H, W, torch.cuda.get_device_name(0)))
        print('labels differing from the kernel\'s, of {}: torch f32 {}, torch bf16 {}'.format(
            total, int((up32 != fused).sum()), int((up16 != fused).sum())))
        print('matrix equal to the kernel\'s: ' + ', '.join('{} {}'.format(k, bool(torch.equal(v, mats['kernel']))) for k, v in mats.items()))
    print('ms per batch, {} alternating repetitions of {} runs'.format(args.reps, args.iters))
    med = {}
    for name in forms:
        med[name] = statistics.median(rows[name])
        print('{:<18} median {:8.4f}   all {}'.format(name, med[name], ' '.join('{:.4f}'.format(v) for v in rows[name])))
    print('kernel / torch f32 (the switch off) = {:.4f};  kernel / torch bf16 = {:.4f}'.format(
        med['kernel'] / med['torch f32'], med['kernel'] / med['torch bf16']))
    if args.forms:
        kernel_forms(logits, targets, (H, W), args.reps, args.iters)


if __name__ == '__main__':
    main()
