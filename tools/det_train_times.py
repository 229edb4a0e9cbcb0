"""The two detection training kernels against their torch-op routes of this same commit, at the Faster R-CNN training shapes:

    matcher    6 images, the 242 991 anchors of an 800 x 1216 batch each, 20 gt boxes each, thresholds 0.3 / 0.7 with low-quality
               matches: `detection.match_boxes` with `host_policy.box_match_hip` on (one sc2_box_match call) and off (the [G, A]
               `box_iou` matrix + `Matcher` per image)
    roi_align  3 072 RoIs over the four pooled maps (200 x 304, 100 x 152, 50 x 76, 25 x 38) of 6 images, C = 256, P = 7, S = 2:
               `detection.multiscale_roi_align` forward + backward with `host_policy.roi_align_bwd_hip` on (sc2_roi_align +
               sc2_roi_align_backward) and off (autograd through the torch-op restatement), plus the backward launch alone

The two forms alternate, R repetitions of K runs between HIP events after a warm-up, medians and the spread (min .. max).  Needs
no data: random boxes, random maps.

    python tools/det_train_times.py [--reps R] [--iters K]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def compare(torch, forms, reps, iters):
    for fn in forms.values():       # warm-up: code objects, the allocator's blocks
        fn()
        fn()
    rows = {k: [] for k in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            rows[name].append(timed(torch, fn, iters))
    for name, r in rows.items():
        print('  {:<28s} median {:9.3f} ms   ({:.3f} .. {:.3f}, {} x {} runs)'.format(name, statistics.median(r), min(r), max(r), reps, iters))
    return {k: statistics.median(v) for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=5)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import sc2bench_amd as S  # noqa: F401
    from sc2bench_amd import detection, hip
    if not torch.cuda.is_available():
        raise SystemExit('det_train_times: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    n_img, H, W = 6, 800, 1216

    # ---- matcher
    strides = (4, 8, 16, 32, 64)
    maps = [torch.zeros(n_img, 1, -(-H // s), -(-W // s), device=dev) for s in strides]
    anchors = detection.AnchorGenerator(((32,), (64,), (128,), (256,), (512,)), ((0.5, 1.0, 2.0),) * 5)(
        detection.ImageList(torch.zeros(n_img, 3, H, W, device=dev), [(H, W)] * n_img), maps)
    gts = []
    for _ in range(n_img):
        xy = torch.rand(20, 2, generator=g) * torch.tensor([W - 64.0, H - 64.0])
        wh = 16 + torch.rand(20, 2, generator=g) ** 2 * 400
        gts.append(torch.cat([xy, torch.min(xy + wh, torch.tensor([float(W), float(H)]))], 1).to(dev))

    def match(on):
        def run():
            hip.configure(box_match_hip=on)
            return detection.match_boxes(gts, anchors, 0.7, 0.3, True)
        return run
    a, b = match(True)(), match(False)()
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    print('matcher: {} images x {} anchors x 20 gt boxes, 0.3 / 0.7, low-quality matches on; device {}'.format(
        n_img, anchors[0].shape[0], torch.cuda.get_device_name(0)))
    print('  matches of the two routes identical: {}; matched anchors per image: {}'.format(same, [int((m >= 0).sum()) for m in a]))
    compare(torch, {'torch ops (matrix + Matcher)': match(False), 'kernel (sc2_box_match)': match(True)}, args.reps, args.iters)
    hip.configure(box_match_hip=hip.HostPolicy.box_match_hip)

    # ---- RoIAlign forward + backward
    K, C, P, Sr = 3072, 256, 7, 2
    sizes = [(-(-H // s), -(-W // s)) for s in strides[:4]]
    scales = [1.0 / s for s in strides[:4]]
    side = 16 * 2 ** (torch.rand(K, generator=g) * 5.2)                     # 16 .. 590 px, log-uniform
    asp = 2 ** (torch.rand(K, generator=g) * 2 - 1)
    wh = torch.stack([side * asp.sqrt(), side / asp.sqrt()], 1)
    xy = torch.rand(K, 2, generator=g) * (torch.tensor([float(W), float(H)]) - wh).clamp(min=0)
    boxes = torch.cat([xy, torch.min(xy + wh, torch.tensor([float(W), float(H)]))], 1)
    img = torch.arange(K) % n_img
    rois = torch.cat([img[:, None].float(), boxes], 1).to(dev)
    levels = detection.LevelMapper(2, 5)([boxes]).to(dev)
    feats = [torch.randn(n_img, C, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for h, w in sizes]
    grad = torch.randn(K, C, P, P, generator=g).to(dev)

    def roi(on, backward=True):
        def run():
            hip.configure(roi_align_bwd_hip=on)
            for f in feats:
                f.grad = None
            out = detection.multiscale_roi_align(feats, scales, rois, levels, P, Sr)
            if backward:
                out.backward(grad)
            return out
        return run
    roi(True)()
    kernel_grads = [f.grad.clone() for f in feats]
    roi(False)()
    print('roi_align: {} RoIs (per level {}), C = {}, P = {}, S = {}, maps {} of {} images'.format(
        K, torch.bincount(levels, minlength=4).tolist(), C, P, Sr, sizes, n_img))
    print('  gradients of the two routes: max |diff| per map {}'.format(
        ['{:.2e}'.format((f.grad - k).abs().max().item()) for f, k in zip(feats, kernel_grads)]))
    l32 = levels.to(torch.int32).contiguous()

    def bwd_alone():
        return hip.roi_align_backward(grad, sizes, scales, rois, l32, n_img, Sr)
    compare(torch, {'torch ops, forward': roi(False, False), 'kernel, forward': roi(True, False),
                    'torch ops, forward + backward': roi(False), 'kernels, forward + backward': roi(True),
                    'sc2_roi_align_backward alone': bwd_alone}, args.reps, args.iters)
    hip.configure(roi_align_bwd_hip=hip.HostPolicy.roi_align_bwd_hip)


if __name__ == '__main__':
    main()
