"""The ImageNet input chains of one batch -- 256 synthetic 375 x 500 RGB sources (already decoded: the JPEG decode stays in the worker on
either path and is not part of either number) to the [256,3,224,224] float32 batch on the device -- on the two paths, in three forms:

    eval       Resize(256) -> CenterCrop([224, 224]) -> ToTensor -> Normalize
    train      RandomResizedCrop([224, 224]) -> RandomHorizontalFlip(0.5) -> ToTensor -> Normalize, seeded draws
    oversize   the eval form with one 1100 x 1500 source among the 256 (past sc2_cls_input's ratio cap: finished by Pillow in the worker)

and per form
    (a) host path     `Compose.__call__` per sample (Pillow + ToTensor + Normalize), `default_collate`, `.to(device)` and a synchronise:
                      wall clock per batch on ONE core.  A loader with W workers divides the per-sample part by at most W.
    (b) plan + pack   `Compose.plan` per sample and `cls_collate_fn`'s packing (what is left for the workers): wall clock, one core.
    (c) materialize   `DeferredClsBatch.materialize(device)`: the copy up, the launch, the status read-back; wall clock around a call
                      that ends in that read-back (a synchronise).
    (d) launch        the sc2_cls_input launch alone, by HIP events (hip.KernelTimer).
(a) and (b) + (c) alternate batch by batch in one process, so both see the same machine; medians over the repetitions.  The outputs of
the two paths are compared bit for bit before anything is timed.  Needs no data.

    python tools/cls_input_times.py [--reps R] [--images N] [--step-timeout S]

Each form is one step in a child process of its own under its own time limit; a step that fails ends the run.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ('eval', 'train', 'oversize')
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


def _row(name, rows):
    return '{:<26s} median {:9.3f}   min {:9.3f}   max {:9.3f}'.format(name, statistics.median(rows), min(rows), max(rows))


def step(args):
    import random
    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    import sc2bench_amd as S  # noqa: F401
    from sc2bench_amd import hip, transforms as T
    if not torch.cuda.is_available():
        raise SystemExit('cls_input_times: no HIP device (times are measured on the GPU or not at all)')
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    form = args.step
    rng = np.random.RandomState(0)
    # (random bytes: neither Pillow's resize nor the kernel takes a time that depends on the content)
    images = [Image.fromarray(rng.randint(0, 256, (375, 500, 3)).astype(np.uint8)) for _ in range(args.images)]
    if form == 'oversize':
        images[len(images) // 2] = Image.fromarray(rng.randint(0, 256, (1100, 1500, 3)).astype(np.uint8))
    if form == 'train':
        chain = T.Compose([T.RandomResizedCrop([224, 224]), T.RandomHorizontalFlip(0.5), T.ToTensor(), T.Normalize(MEAN, STD)])
    else:
        chain = T.Compose([T.Resize(256), T.CenterCrop([224, 224]), T.ToTensor(), T.Normalize(MEAN, STD)])
    labels = list(range(len(images)))

    def host_batch(k):
        random.seed(k)
        batch, _ = torch.utils.data.default_collate([(chain(image), label) for image, label in zip(images, labels)])
        return batch.to(dev, non_blocking=True)

    def planned_batch(k):
        random.seed(k)
        return T.cls_collate_fn([(chain.plan(image), label) for image, label in zip(images, labels)])[0]

    hip.configure(cls_input_hip=True)
    for k in range(2):      # bit for bit, and the warm-up of the code object and the allocator's blocks
        want, got = host_batch(k), planned_batch(k).materialize(dev)
        assert torch.equal(got, want), 'the two paths differ on batch {}'.format(k)
    a_rows, b_rows, c_rows = [], [], []
    kept = None
    for k in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_batch(k)
        torch.cuda.synchronize()
        a_rows.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        batch = planned_batch(k)
        t1 = time.perf_counter()
        batch.materialize(dev)      # (ends in the read-back of the status words)
        t2 = time.perf_counter()
        b_rows.append((t1 - t0) * 1e3)
        c_rows.append((t2 - t1) * 1e3)
        kept = batch
    with hip.KernelTimer(select=lambda tag: tag == 'cls_input') as timer:
        for _ in range(20):
            kept.materialize(dev)
    torch.cuda.synchronize()
    hip.configure(cls_input_hip=hip.HostPolicy.cls_input_hip)
    sums = [b + c for b, c in zip(b_rows, c_rows)]
    print('form {}: {} sources of 375 x 500 -> [{},3,224,224] f32 on {} (clocks and power as the machine sets them: nothing changed), host '
          'one core of {}; ms per batch over {} alternating batches'.format(form, args.images, args.images, torch.cuda.get_device_name(0),
                                                                          _cpu_name(), args.reps))
    print('outputs equal bit for bit on 2 batches; fallbacks {}; stored boxes {:.2f} MB per batch against {:.2f} MB of float32'.format(
        T.DeferredClsBatch.fallbacks, kept.buf.numel() / 1e6, args.images * 3 * 224 * 224 * 4 / 1e6))
    print(_row('(a) host path', a_rows))
    print(_row('(b) plan + pack', b_rows))
    print(_row('(c) materialize', c_rows))
    print(_row('(b) + (c)', sums))
    for tag, (count, ms) in sorted(timer.summary().items()):
        print('(d) the launch alone ({}): {:.4f} ms (mean of {})'.format(tag, ms, count))
    print('(a) / ((b) + (c)) = {:.2f}'.format(statistics.median(a_rows) / statistics.median(sums)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--step', choices=STEPS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    for name in STEPS:      # one child per step, each under its own limit; nothing more is started after a step that failed
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--step', name, '--reps', str(args.reps),
               '--images', str(args.images)]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit('cls_input_times: step {} ended with status {}'.format(name, rc))


if __name__ == '__main__':
    main()
