"""Development aid: the serial context-model scan of `mbt2018` (csrc/ar_context.hip) -- per-step and per-scan time of compress
and decompress on 256 x 256 inputs (16 x 16 latent = 256 dependent steps), and the resumable rANS decoder's time per symbol.

    python tools/ar_codec_time.py [--quality 8] [--batches 1,16,256] [--size 256] [--scan-precision f32] [--encoder-precision f32]

With --scan-precision f32 every batch is measured twice in the same process, 'bf16' / 'bf16' first, then the modes asked for, and
the ratio of the step times is printed.

Times are HIP-event times of the scan launch alone (the transforms and the coder around it are excluded); `decode - encode`
per step and symbol isolates the serial decode inside the scan.  The stand-alone decoder line decodes the same streams
pixel-major, one launch of M symbols per step as the scan would, and reports the mean time per symbol."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc2bench_amd as S  # noqa: E402
from sc2bench_amd import hip  # noqa: E402


def event_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quality', type=int, default=8)
    ap.add_argument('--batches', default='1,16,256')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--scan-precision', default='bf16', choices=['bf16', 'f32'],
                    help="'f32': also time the f32 scan (sc2_ar_scan_f32) and print it beside the 'bf16' figures of the same run")
    ap.add_argument('--encoder-precision', default='bf16', choices=['bf16', 'f32', 'bf16x3', 'bf16x6'],
                    help='the transforms that make y and p1 for the second measurement (a precise mode needs --scan-precision f32)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = S.mbt2018(quality=args.quality).eval().to(dev)
    with torch.no_grad():
        m.g_a[6].weight.mul_(8.0)
    m.update()
    M = m.M
    print('mbt2018 q{} (N={}, M={}), {}x{} input'.format(args.quality, m.N, M, args.size, args.size))
    for B in [int(b) for b in args.batches.split(',')]:
        x = torch.rand(B, 3, args.size, args.size, device=dev)
        base = scan_times(m, x, 'bf16', 'bf16', args.iters, resume=True)
        if args.scan_precision != 'bf16':
            # the same process, the same images: the 'bf16' figures above are the ones to read these beside
            t = scan_times(m, x, args.scan_precision, args.encoder_precision, args.iters)
            print('        {} / bf16: encode step x{:.3f}, decode step x{:.3f}'.format(
                args.scan_precision, t[0] / base[0], t[1] / base[1]), flush=True)


def scan_times(m, x, scan_precision, encoder_precision, iters, resume=False):
    """-> (encode ms, decode ms) of one scan launch in the given modes; prints the line.  The model is left 'bf16' / 'bf16'."""
    dev = x.device
    gc = m.gaussian_conditional
    M, B = m.M, x.shape[0]
    m.set_encoder_precision('bf16').set_scan_precision(scan_precision).set_encoder_precision(encoder_precision)
    try:
        with torch.no_grad():
            enc = m.compress_device(x)
            obj = m.compress(x)
            p1, y_pad = m._scan_inputs(m._z_hat_nhwc(obj['strings'][1], obj['shape']))
        w = m._scan_weights()
    finally:
        m.set_encoder_precision('bf16').set_scan_precision('bf16')
    _, H, W, _ = p1.shape
    steps = H * W
    table = gc.scale_table.float().contiguous()
    sym, idx = torch.empty_like(enc['symbols']), torch.empty_like(enc['indexes'])
    y = enc['y'].float().contiguous()

    def run_enc():
        y_pad.zero_()
        hip.ar_scan(w, p1, y_pad, None, table, gc._scale_bound, y=y, symbols=sym, indexes=idx)

    buf, off, nb = gc.pack_strings(obj['strings'][0], dev)
    cdf, cdf_len, offset = gc._tables()
    dec = {'buf': buf, 'off': off, 'nb': nb, 'cdfs': cdf, 'cdf_sizes': cdf_len.int().contiguous(),
           'offsets': offset.int().contiguous(), 'cdf_entries': int(cdf_len.sum().item()) - cdf_len.numel(),
           'st_x': torch.zeros(B, dtype=torch.int64, device=dev), 'st_pos': torch.zeros(B, dtype=torch.int32, device=dev),
           'status': torch.zeros(B, dtype=torch.int32, device=dev)}
    y_hat = torch.empty((B, H, W, M), dtype=torch.bfloat16, device=dev)

    def run_dec():
        y_pad.zero_()
        hip.ar_scan(w, p1, y_pad, y_hat, table, gc._scale_bound, decode=dec)

    t_enc = event_ms(run_enc, iters)
    t_dec = event_ms(run_dec, iters)
    assert int(dec['status'].max()) == 0, 'decode status {}'.format(dec['status'].tolist())
    assert torch.equal(y_pad, enc['y_hat_pad']), 'decoded y_hat differs from the encoder'
    line = ('B={:4d}  scan {:>4} encoder {:>6}  steps={}  encode scan {:9.3f} ms ({:7.2f} us/step)  decode scan {:9.3f} ms ({:7.2f} '
            'us/step, decode share {:6.1f} ns/symbol)'.format(B, scan_precision, encoder_precision, steps, t_enc, t_enc / steps * 1e3,
                                                              t_dec, t_dec / steps * 1e3, (t_dec - t_enc) / (steps * M) * 1e6))
    if resume:
        # stand-alone resumable decoder: one launch of M symbols per step
        idx_steps = enc['indexes'].view(B, steps, M)

        def run_resume():
            st = None
            for p in range(steps):
                _, st = hip.rans_decode_resume(buf, off, nb, idx_steps[:, p].contiguous(), cdf, dec['cdf_sizes'], dec['offsets'],
                                               state=st, last=p == steps - 1)
            return st
        t_res = event_ms(run_resume, 1)
        line += '  resumable decoder {:7.1f} ns/symbol/stream ({:7.2f} us/step incl. launch)'.format(
            t_res / (steps * M) * 1e6, t_res / steps * 1e3)
    print(line, flush=True)
    return t_enc, t_dec


if __name__ == '__main__':
    main()
