"""The PASCAL train augmentation of one batch -- 16 synthetic 375 x 500 RGB sources with their masks through CustomRandomResize(256, 1026)
-> CustomRandomHorizontalFlip(0.5) -> CustomRandomCrop(513) -> CustomToTensor -> CustomNormalize -- in its two forms, on the same seeded
draws:

    host      `CustomCompose.__call__` per sample (Pillow + torch) and the collate function, on ONE core: wall clock per batch.  A data
              loader with W workers divides this by at most W.
    device    `CustomCompose.plan` per sample and the collate function's packing (what is left for the workers: wall clock, one core),
              then `DeferredSegBatch.materialize`: one copy up, sc2_seg_augment's two launches, the status read-back -- HIP events
              around K batches after warm-up -- and the two launches alone (an event pair around the library call).

The outputs of the two forms are compared bit for bit before anything is timed.  Needs no data.

    python tools/seg_augment_times.py [--reps R] [--iters K] [--images N] [--step-timeout S]

Each form is one step in a child process of its own under its own time limit; a step that fails ends the run.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ('host', 'device')
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _cpu_name():
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown CPU'


def _setup(args):
    import random
    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    import sc2bench_amd as S  # noqa: F401
    from sc2bench_amd import transforms as T
    torch.set_num_threads(1)
    rng = np.random.RandomState(0)
    pairs = []
    for _ in range(args.images):
        # (random bytes: neither Pillow's resize nor the kernels take a time that depends on the content)
        image = rng.randint(0, 256, (375, 500, 3)).astype(np.uint8)
        mask = rng.randint(0, 22, (375, 500)).astype(np.uint8)
        mask[mask == 21] = 255
        pairs.append((Image.fromarray(image), Image.fromarray(mask)))
    chain = T.CustomCompose([T.CustomRandomResize(256, 1026), T.CustomRandomHorizontalFlip(0.5), T.CustomRandomCrop(513),
                             T.CustomToTensor(), T.CustomNormalize(MEAN, STD)])

    def seed(k):
        random.seed(k)
        torch.manual_seed(k)

    def host_batch(k):
        seed(k)
        return T.pascal_seg_eval_collate_fn([chain(image, mask) for image, mask in pairs])

    def planned_batch(k):
        seed(k)
        return T.pascal_seg_eval_collate_fn([(chain.plan(image, mask), None) for image, mask in pairs])

    return torch, T, host_batch, planned_batch


def step_host(args):
    torch, T, host_batch, planned_batch = _setup(args)
    host_batch(0)
    rows = []
    for k in range(args.reps * args.iters):
        t0 = time.perf_counter()
        host_batch(k)
        rows.append((time.perf_counter() - t0) * 1e3)
    print('host form, {} images 375 x 500 -> 513 x 513 per batch, one core of {}: ms per batch over {} batches'.format(
        args.images, _cpu_name(), len(rows)))
    print('host     median {:9.3f}   min {:9.3f}   max {:9.3f}'.format(statistics.median(rows), min(rows), max(rows)))


def step_device(args):
    torch, T, host_batch, planned_batch = _setup(args)
    from sc2bench_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit('seg_augment_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    hip.configure(seg_augment_hip=True)
    for k in range(3):      # bit for bit, and the warm-up of the code objects and the allocator's blocks
        want, got = host_batch(k), planned_batch(k).materialize(dev)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), 'the two forms differ on batch {}'.format(k)
    plan_rows = []
    batches = []
    for k in range(args.iters):
        t0 = time.perf_counter()
        batches.append(planned_batch(k))
        plan_rows.append((time.perf_counter() - t0) * 1e3)
    rows = []
    for _ in range(args.reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for b in batches:
            b.materialize(dev)
        stop.record()
        torch.cuda.synchronize()
        rows.append(start.elapsed_time(stop) / len(batches))
    with hip.KernelTimer(select=lambda tag: tag == 'seg_augment') as timer:
        for b in batches:
            b.materialize(dev)
    torch.cuda.synchronize()
    hip.configure(seg_augment_hip=hip.HostPolicy.seg_augment_hip)
    print('device form, {} images 375 x 500 -> 513 x 513 per batch, device {} (clocks and power as the machine sets them: nothing '
          'changed), host one core of {}'.format(args.images, torch.cuda.get_device_name(0), _cpu_name()))
    print('outputs equal the host form bit for bit on 3 batches; fallbacks {}'.format(T.DeferredSegBatch.fallbacks))
    print('plan + pack on the host (wall clock, one core), ms per batch over {} batches'.format(len(plan_rows)))
    print('plan     median {:9.3f}   min {:9.3f}   max {:9.3f}'.format(statistics.median(plan_rows), min(plan_rows), max(plan_rows)))
    print('materialize = copy up ({:.2f} MB pageable) + two launches + status read-back, HIP events, ms per batch, {} repetitions of {} batches'.format(
        batches[0].buf.numel() / 1e6, args.reps, len(batches)))
    print('device   median {:9.3f}   min {:9.3f}   max {:9.3f}   all {}'.format(statistics.median(rows), min(rows), max(rows),
                                                                            ' '.join('{:.3f}'.format(v) for v in rows)))
    for tag, (count, ms) in sorted(timer.summary().items()):
        print('the two launches alone ({}): {:.4f} ms (mean of {})'.format(tag, ms, count))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--images', type=int, default=16)
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--step', choices=STEPS)
    args = ap.parse_args()
    if args.step:
        return {'host': step_host, 'device': step_device}[args.step](args)
    for name in STEPS:      # one child per step, each under its own limit; nothing more is started after a step that failed
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--step', name, '--reps', str(args.reps),
               '--iters', str(args.iters), '--images', str(args.images)]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit('seg_augment_times: step {} ended with status {}'.format(name, rc))


if __name__ == '__main__':
    main()
