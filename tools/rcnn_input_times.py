"""The detection input-compression baseline's input side alone -- `detection.RCNNTransformWithCompression.forward` (resize to
800 x 1066, JPEG at quality 90, normalise, zero-padded batch) on float images that are on the device already, as
`wrapper.InputCompressionDetectionModel` runs it in front of Faster R-CNN -- in two forms, alternating in one process, R repetitions,
wall clock around K runs with a device synchronisation (the host path is host work):

    host      `host_policy.rcnn_input_hip = False`: per image torch's interpolate, `mul(255).byte()`, the copy to the host, Pillow
              save / open, ToTensor, the copy back, normalise, and the padded batch
    kernel    `host_policy.rcnn_input_hip = True`: per image sc2_rcnn_resize_u8, the three launches of sc2_jpeg_image_codec and
              sc2_rcnn_normalize_pad; one read-back of sizes and status words per list

at one image per call (the reference config's batch size) and at a list of six, and the two new kernels alone by HIP events.
Medians and their ratio.  The two forms' image sizes, batch shapes and file sizes are compared first (sizes: within a few percent --
the resized bytes of the two forms may differ by one where the exact value all but touches an integer, tests/ref_rcnn_input.py).
Needs no data: natural-looking synthetic images, a smooth gradient plus noise.

    python tools/rcnn_input_times.py [--reps R] [--iters K] [--lists 1,6] [--out FILE]
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

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


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


def synthetic_images(n, H, W, seed, dev):
    """n float images [3,H,W] in [0, 1] on `dev`: per channel a gradient across the image plus Gaussian noise"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    images = []
    for _ in range(n):
        planes = []
        for c in range(3):
            a, b, base = rng.uniform(-120, 120), rng.uniform(-120, 120), rng.uniform(60, 190)
            planes.append(base + a * (xx / (W - 1) - 0.5) + b * (yy / (H - 1) - 0.5) + rng.normal(0.0, 6.0, (H, W)))
        u8 = np.clip(np.rint(np.stack(planes)), 0, 255).astype(np.uint8)
        images.append(torch.from_numpy(u8).to(torch.float32).div(255).to(dev))
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--lists', default='1,6')
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--out', help='also write the report to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rcnn_input_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    codec = S.transforms.Compose([S.PILImageModule(returns_file_size=True, format='JPEG', quality=args.quality)])
    transform = S.RCNNTransformWithCompression(S.GeneralizedRCNNTransform(800, 1333, MEAN, STD), dev, codec,
                                               [{'key': 'FileSizeAccumulator', 'kwargs': {'unit': 'B'}}]).eval()
    transform.activate_analysis()
    oh, ow = transform.resized_size(args.height, args.width)
    say('RCNNTransformWithCompression, JPEG quality {}, {}x{} -> {}x{}, device {}'.format(
        args.quality, args.height, args.width, oh, ow, torch.cuda.get_device_name(0)))
    say('ms per call, {} alternating repetitions of {} runs (wall clock, synchronised); kernels alone by HIP events'.format(args.reps, args.iters))
    for n in (int(v) for v in args.lists.split(',')):
        images = synthetic_images(n, args.height, args.width, seed=n, dev=dev)

        def form(on):
            def run():
                hip.configure(rcnn_input_hip=on)
                transform.clear_analysis()
                out = transform(images)[0]
                return out, list(transform.analyzers[0].file_size_list)
            return run
        forms = {'host': form(False), 'kernel': form(True)}
        with torch.no_grad():
            (x_host, s_host), (x_kernel, s_kernel) = forms['host'](), forms['kernel']()      # (also the warm-up)
            assert x_host.image_sizes == x_kernel.image_sizes and x_host.tensors.shape == x_kernel.tensors.shape
            assert len(s_host) == len(s_kernel) == n and all(abs(a - b) <= 0.05 * a for a, b in zip(s_host, s_kernel)), (s_host, s_kernel)
            differ = (x_host.tensors != x_kernel.tensors).float().mean().item()
            rows = {name: [] for name in forms}
            for _ in range(args.reps):
                for name, fn in forms.items():
                    rows[name].append(wall_ms(fn, args.iters))
        med = {name: statistics.median(v) for name, v in rows.items()}
        say('list of {}: batch {}  mean size host {:.0f} B, kernel {:.0f} B  elements that differ {:.4f}'.format(
            n, tuple(x_kernel.tensors.shape), sum(s_host) / n, sum(s_kernel) / n, differ))
        for name in forms:
            say('  {:<13} median {:10.3f}   all {}'.format(name, med[name], ' '.join('{:.3f}'.format(v) for v in rows[name])))
        say('  kernel / host = {:.4f}'.format(med['kernel'] / med['host']))
    image = synthetic_images(1, args.height, args.width, seed=0, dev=dev)[0]
    pixels, status = hip.rcnn_resize_u8(image, oh, ow)
    slot = torch.empty((3, -(-oh // 32) * 32, -(-ow // 32) * 32), dtype=torch.float32, device=dev)
    alone = {'rcnn_resize_u8': lambda: hip.rcnn_resize_u8(image, oh, ow, out=pixels, status=status),
             'jpeg_image_codec': lambda: hip.jpeg_image_codec(pixels.unsqueeze(0), args.quality),
             'rcnn_normalize_pad': lambda: hip.rcnn_normalize_pad(pixels, MEAN, STD, slot)}
    for name, fn in alone.items():
        fn()
        times = [event_ms(fn, 20) for _ in range(args.reps)]
        say('  {:<19} alone, median {:8.4f}   all {}'.format(name, statistics.median(times), ' '.join('{:.4f}'.format(v) for v in times)))
    hip.configure(rcnn_input_hip=hip.HostPolicy.rcnn_input_hip)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
