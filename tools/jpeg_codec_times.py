"""The codec feature-compression baseline alone -- `transforms.PILTensorModule(format='JPEG', quality=90).forward_batch` on a feature map
of BASELINE config 1 (ResNet-50 split behind layer2: [B,512,28,28]) and of a split behind layer1 ([B,256,56,56]) -- in two forms,
alternating in one process, R repetitions, wall-clock around K runs with a device synchronisation (the host path is host work):

    host      `host_policy.jpeg_codec_hip = False`: per sample and channel group, torch reductions, Pillow save / open, copies both ways
    kernel    `host_policy.jpeg_codec_hip = True`: one sc2_jpeg_tensor_codec launch and one device-to-host read per batch

and the kernel alone by HIP events (no read back).  Medians and their ratio; the two forms' features and sizes are compared first.
Needs no data: ReLU-like random features.

    python tools/jpeg_codec_times.py [--reps R] [--iters K] [--batches 1,32]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc2bench_amd as S  # noqa: E402
from sc2bench_amd import hip  # noqa: E402


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def event_ms(fn, iters):
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--batches', default='1,32')
    ap.add_argument('--quality', type=int, default=90)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_codec_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    module = S.PILTensorModule(returns_file_size=True, format='JPEG', quality=args.quality)
    print('JPEG feature codec at quality {}, device {}'.format(args.quality, torch.cuda.get_device_name(0)))
    print('ms per batch, {} alternating repetitions of {} runs (wall clock, synchronised); kernel alone by HIP events'.format(args.reps, args.iters))
    gen = torch.Generator().manual_seed(0)
    for C, H, W in ((512, 28, 28), (256, 56, 56)):
        for B in (int(v) for v in args.batches.split(',')):
            x = (torch.randn(B, C, H, W, generator=gen).clamp_min(0) * 2 + 0.01 * torch.rand(B, C, 1, 1, generator=gen)).to(dev)

            def form(on):
                def run():
                    hip.configure(jpeg_codec_hip=on)
                    return module.forward_batch(x)
                return run
            forms = {'host': form(False), 'kernel': form(True)}
            with torch.no_grad():
                (f_host, s_host), (f_kernel, s_kernel) = forms['host'](), forms['kernel']()      # (also the warm-up)
                same = bool(torch.equal(f_host.view(torch.int32), f_kernel.view(torch.int32))) and s_host == s_kernel
                rows = {name: [] for name in forms}
                for _ in range(args.reps):
                    for name, fn in forms.items():
                        rows[name].append(wall_ms(fn, args.iters))
                alone = [event_ms(lambda: hip.jpeg_tensor_codec(x, args.quality), 10) for _ in range(args.reps)]
            med = {name: statistics.median(v) for name, v in rows.items()}
            print('[{},{},{},{}]  features and sizes equal: {}  mean size {:.0f} B'.format(B, C, H, W, same, sum(s_kernel) / len(s_kernel)))
            for name in forms:
                print('  {:<13} median {:10.3f}   all {}'.format(name, med[name], ' '.join('{:.3f}'.format(v) for v in rows[name])))
            print('  {:<13} median {:10.4f}   all {}'.format('kernel alone', statistics.median(alone), ' '.join('{:.4f}'.format(v) for v in alone)))
            print('  kernel / host = {:.4f}'.format(med['kernel'] / med['host']))
    hip.configure(jpeg_codec_hip=hip.HostPolicy.jpeg_codec_hip)


if __name__ == '__main__':
    main()
