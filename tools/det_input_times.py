"""The detector's input transform of one COCO batch -- six synthetic 480 x 640 RGB sources through ImageToTensor -> flip ->
GeneralizedRCNNTransform(800, 1333) to the padded batch [6,3,800,1088] -- in its two forms, in ONE process, alternating:

    new       the planned batch (`transforms.DeferredDetBatch`): one copy up of the 5.5 MB of source bytes and one sc2_det_input launch
    parent    the float32 list of the host chain (22 MB) copied up image by image, then the transform's torch ops per image
              (normalise, F.interpolate, and the copy into the zero-filled batch)

HIP events around K batches after a warm-up, R alternating repetitions, medians; and the launch alone (an event pair around the
library call).  The host memory is pageable in both forms.  What the loader workers do is outside the timed region in BOTH forms:
decoding and packing the bytes for the new one, decoding plus `to_tensor` and the flip for the parent one (those float32 images are
made once, before the loop) -- the figures are the consumer process's share, not a loader's throughput.  The two outputs are compared against the bound of tests/ref_det_input.py
(2 delta) before anything is timed.  Needs no data.

    python tools/det_input_times.py [--reps R] [--iters K] [--images N] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--out')
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import sc2bench_amd as S
    from sc2bench_amd import hip, transforms as T
    import ref_det_input as RI
    if not torch.cuda.is_available():
        raise SystemExit('det_input_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    # (random bytes: neither form takes a time that depends on the content)
    samples = [T.DeferredDetSample(rng.randint(0, 256, (480, 640, 3)).astype(np.uint8), bool(i % 2)) for i in range(args.images)]
    batch = T.DeferredDetBatch(samples)
    listed = batch.tensors('cpu')
    tr = S.detection.GeneralizedRCNNTransform(800, 1333, list(MEAN), list(STD)).eval()

    fresh = [T.DeferredDetBatch(samples).to(dev) for _ in range(args.iters)]      # one per timed batch: nothing on the device, nothing cached
    turn = [0]

    def new():
        b = fresh[turn[0] % len(fresh)]
        turn[0] += 1
        b.release()      # (host side only: drops the references of the previous round)
        return tr(b)[0].tensors

    def parent():
        return tr([image.to(dev, non_blocking=True) for image in listed])[0].tensors

    hip.configure(det_input_hip=True)
    launches = T.DeferredDetBatch.launches
    a, b = new(), parent()
    assert T.DeferredDetBatch.launches == launches + 1, 'the new form did not take the kernel'
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max())
    bound = 2 * RI.delta(480, 640, MEAN, STD)
    assert err <= bound, 'the two forms differ by {} (2 delta = {})'.format(err, bound)
    for _ in range(3):      # warm-up: code objects, the allocator's blocks
        new()
        parent()
    rows = {'new': [], 'parent': []}
    for _ in range(args.reps):
        for name, form in (('new', new), ('parent', parent)):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(args.iters):
                form()
            stop.record()
            torch.cuda.synchronize()
            rows[name].append(start.elapsed_time(stop) / args.iters)
    with hip.KernelTimer(select=lambda tag: tag == 'det_input') as timer:
        for _ in range(args.iters):
            new()
    torch.cuda.synchronize()
    hip.configure(det_input_hip=hip.HostPolicy.det_input_hip)
    out_bytes = a.numel() * 4
    lines = ['{} sources of 480 x 640 -> {} ({:.1f} MB written), device {} (clocks and power as the machine sets them: nothing changed)'.format(
        args.images, list(a.shape), out_bytes / 1e6, torch.cuda.get_device_name(0)),
        'the two forms differ by at most {:.3e} (2 delta = {:.3e})'.format(err, bound),
        'HIP events, ms per batch, {} alternating repetitions of {} batches, pageable host memory'.format(args.reps, args.iters)]
    for name, what in (('new', 'copy up of {:.2f} MB of bytes + one launch'.format(batch.buf.numel() / 1e6)),
                       ('parent', 'copy up of {:.2f} MB of float32 + torch ops per image'.format(sum(t.numel() for t in listed) * 4 / 1e6))):
        v = rows[name]
        lines.append('{:7s} median {:8.3f}   min {:8.3f}   max {:8.3f}   ({})'.format(name, statistics.median(v), min(v), max(v), what))
    for tag, (count, ms) in sorted(timer.summary().items()):
        lines.append('the launch alone ({}): {:.4f} ms (mean of {}), {:.2f} TB/s written'.format(tag, ms, count, out_bytes / ms / 1e9))
    lines.append('ratio parent / new (medians): {:.2f}'.format(statistics.median(rows['parent']) / statistics.median(rows['new'])))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
