"""The codec input-compression baseline's input side alone -- `transforms.PILImageModule(format='JPEG', quality=90).forward_batch` on a
list of 224 x 224 RGB images, then `ToTensor` + `Normalize` to the classifier's input on the device, as
`wrapper.CodecInputCompressionClassifier` runs them -- in two forms, alternating in one process, R repetitions, wall-clock around K runs
with a device synchronisation (the host path is host work):

    host      `host_policy.jpeg_image_hip = False`: per image Pillow save / open, ToTensor and Normalize on the host, one copy to the
              device per batch
    kernel    `host_policy.jpeg_image_hip = True`: the images stacked and copied up once, the three launches of sc2_jpeg_image_codec,
              one device-to-host read of the sizes, ToTensor and Normalize on the batch on the device

and the kernels alone by HIP events (pixels on the device already, no read back).  Medians and their ratio; the two forms' outputs
and sizes are compared first.  Needs no data: natural-looking synthetic images, a smooth gradient plus noise.

    python tools/jpeg_image_times.py [--reps R] [--iters K] [--batches 1,256]
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


def synthetic_images(B, H, W, seed):
    """B PIL RGB images: per channel a gradient across the image plus Gaussian noise, different for every image"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    images = []
    for _ in range(B):
        planes = []
        for c in range(3):
            a, b, base = rng.uniform(-120, 120), rng.uniform(-120, 120), rng.uniform(60, 190)
            planes.append(base + a * (xx / (W - 1) - 0.5) + b * (yy / (H - 1) - 0.5) + rng.normal(0.0, 6.0, (H, W)))
        images.append(Image.fromarray(np.clip(np.rint(np.stack(planes, axis=2)), 0, 255).astype(np.uint8)))
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--batches', default='1,256')
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--side', type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_image_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    T = S.transforms
    module = S.PILImageModule(returns_file_size=True, format='JPEG', quality=args.quality)
    post = T.Compose([T.ToTensor(), T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    print('JPEG input codec at quality {}, device {}'.format(args.quality, torch.cuda.get_device_name(0)))
    print('ms per batch, {} alternating repetitions of {} runs (wall clock, synchronised); kernels alone by HIP events'.format(args.reps, args.iters))
    for B in (int(v) for v in args.batches.split(',')):
        images = synthetic_images(B, args.side, args.side, seed=B)

        def form(on):
            def run():
                hip.configure(jpeg_image_hip=on)
                decoded, sizes = module.forward_batch(images, dev)
                if isinstance(decoded, torch.Tensor):
                    return post(decoded), sizes
                return torch.stack([post(d) for d in decoded]).to(dev), sizes
            return run
        forms = {'host': form(False), 'kernel': form(True)}
        with torch.no_grad():
            (x_host, s_host), (x_kernel, s_kernel) = forms['host'](), forms['kernel']()      # (also the warm-up)
            assert x_host.device == x_kernel.device and x_host.shape == x_kernel.shape == (B, 3, args.side, args.side)
            assert torch.equal(x_host, x_kernel), 'the two forms give different classifier inputs'
            assert s_host == s_kernel, 'the two forms report different file sizes'
            rows = {name: [] for name in forms}
            for _ in range(args.reps):
                for name, fn in forms.items():
                    rows[name].append(wall_ms(fn, args.iters))
            x_dev = torch.from_numpy(np.stack([np.asarray(img) for img in images])).to(dev).permute(0, 3, 1, 2)
            alone = [event_ms(lambda: hip.jpeg_image_codec(x_dev, args.quality), 10) for _ in range(args.reps)]
        med = {name: statistics.median(v) for name, v in rows.items()}
        print('[{},3,{},{}]  inputs and sizes equal: True  mean size {:.0f} B'.format(B, args.side, args.side, sum(s_kernel) / len(s_kernel)))
        for name in forms:
            print('  {:<13} median {:10.3f}   all {}'.format(name, med[name], ' '.join('{:.3f}'.format(v) for v in rows[name])))
        print('  {:<13} median {:10.4f}   all {}'.format('kernels alone', statistics.median(alone), ' '.join('{:.4f}'.format(v) for v in alone)))
        print('  kernel / host = {:.4f}'.format(med['kernel'] / med['host']))
    hip.configure(jpeg_image_hip=hip.HostPolicy.jpeg_image_hip)


if __name__ == '__main__':
    main()
