"""The segmentation training loss alone -- low-resolution logits of both heads -> 1.0 CE(out) + 0.5 CE(aux) at the input's size, forward
and backward to the logits -- at the PASCAL stage-2 shape: 8 x 21 x 65 x 65 -> 513 x 513, f32 and bf16 logits, int64 targets with
the ignore label 255.  Two forms on the same tensors, alternating, R repetitions in one process, HIP events around K runs:

    torch     `host_policy.seg_loss_hip = False`: F.interpolate + F.cross_entropy + autograd per head
    kernels   `host_policy.seg_loss_hip = True`: sc2_seg_ce_forward + sc2_seg_ce_backward per head (dense.seg_cross_entropy)

with the medians, the spread (min .. max), the peak of allocated bytes above the inputs, how far the two forms' losses and
gradients are apart, and the mean time of the forward (two launches) and backward (one launch) library calls of one head.  Needs no data: random logits, random targets.

    python tools/seg_loss_times.py [--reps R] [--iters K] [--images N] [--step-timeout S]

Each dtype is one step in a child process of its own under its own time limit; a step that fails ends the run.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ('float32', 'bfloat16')


def step(dtype_name, args):
    import torch
    sys.path.insert(0, ROOT)
    import sc2bench_amd as S  # noqa: F401
    from sc2bench_amd import dense, hip
    if not torch.cuda.is_available():
        raise SystemExit('seg_loss_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    dtype = getattr(torch, dtype_name)
    n, c, h, w, H, W = args.images, 21, 65, 65, 513, 513
    g = torch.Generator().manual_seed(0)
    heads = [(torch.randn(n, c, h, w, generator=g).to(dtype).to(dev).requires_grad_(True), weight) for weight in (1.0, 0.5)]
    targets = torch.randint(0, c + 1, (n, H, W), generator=g)
    targets[targets == c] = 255
    targets = targets.to(dev)

    def form(on):
        def run():
            hip.configure(seg_loss_hip=on)
            for x, _ in heads:
                x.grad = None
            loss = sum(weight * dense.seg_cross_entropy(x, (H, W), targets) for x, weight in heads)
            loss.backward()
            return loss
        return run

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.iters

    forms = {'torch': form(False), 'kernels': form(True)}
    rows, peaks, results = {k: [] for k in forms}, {}, {}
    for name, fn in forms.items():      # warm-up: code objects, the allocator's blocks; then the peak of one run
        fn()
        fn()
        torch.cuda.synchronize()
        for x, _ in heads:
            x.grad = None
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        results[name] = (loss.item(), [x.grad.float().clone() for x, _ in heads])
    for _ in range(args.reps):
        for name, fn in forms.items():
            rows[name].append(timed(fn))
    hip.configure(seg_loss_hip=hip.HostPolicy.seg_loss_hip)
    print('segmentation loss, forward + backward, out + aux at 1.0 / 0.5: {} x {} x {} x {} -> {} x {}, {} logits, device {}'.format(
        n, c, h, w, H, W, dtype_name, torch.cuda.get_device_name(0)))
    print('loss: torch {:.7f}, kernels {:.7f};  max |gradient difference| {:.3e} (largest |gradient| {:.3e})'.format(
        results['torch'][0], results['kernels'][0],
        max(float((a - b).abs().max()) for a, b in zip(results['torch'][1], results['kernels'][1])),
        max(float(a.abs().max()) for a in results['torch'][1])))
    print('ms per step, {} alternating repetitions of {} runs'.format(args.reps, args.iters))
    med = {}
    for name in forms:
        med[name] = statistics.median(rows[name])
        print('{:<8} median {:8.4f}   min {:8.4f}   max {:8.4f}   peak allocated above the inputs {:7.1f} MB   all {}'.format(
            name, med[name], min(rows[name]), max(rows[name]), peaks[name] / 1e6, ' '.join('{:.4f}'.format(v) for v in rows[name])))
    print('kernels / torch = {:.4f}'.format(med['kernels'] / med['torch']))
    with hip.KernelTimer(select=lambda tag: tag.startswith('seg_ce_')) as timer:      # an event pair around each library call
        for _ in range(args.iters):
            forms['kernels']()
    torch.cuda.synchronize()
    hip.configure(seg_loss_hip=hip.HostPolicy.seg_loss_hip)
    print('per library call (one head): ' + ', '.join('{} {:.4f} ms (mean of {})'.format(tag, ms, count)
                                                      for tag, (count, ms) in sorted(timer.summary().items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--step-timeout', type=int, default=120)
    ap.add_argument('--step', choices=STEPS)
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    for name in STEPS:      # one child per step, each under its own limit; nothing more is started after a step that failed
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--step', name, '--reps', str(args.reps),
               '--iters', str(args.iters), '--images', str(args.images)]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit('seg_loss_times: step {} ended with status {}'.format(name, rc))


if __name__ == '__main__':
    main()
