"""The four encoder precisions side by side on one box, in one process: the bench model at bs 256, 224 x 224.

    python tools/encoder_modes.py [--rounds 3] [--reps 5] [--launches]

The modes ('bf16', 'f32', 'bf16x3', 'bf16x6') are ALTERNATED for --rounds rounds, so that clock and thermal drift fall on all of
them alike.  Per mode: the `stage_front` time per batch of every round (HIP events, as bench.py's precision_check), the symbol
mismatch against the oracle's f32 CPU encoder on the first 64 images, the images whose symbols are all identical, and the bpp of
the streams the device codes from them.  --launches adds the per-launch times of one extra pass (hip.KernelTimer).
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from sc2bench_amd import hip  # noqa: E402

MODES = ('bf16', 'f32', 'bf16x3', 'bf16x6')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5, help='stage_front calls per timed interval')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--launches', action='store_true')
    args = ap.parse_args()
    assert args.rounds >= 3
    dev = torch.device('cuda:0')
    model = bench.build_model(dev)
    x = bench.synthetic_batch(args.batch, dev)
    n = min(64, args.batch)
    ref = bench.oracle_model(model.state_dict())
    eb, reb = model.bottleneck_layer.entropy_bottleneck, ref.bottleneck_layer.entropy_bottleneck
    xc = x[:n].float().cpu()
    pix = x.shape[-1] * x.shape[-2]
    with torch.no_grad():
        ref_sym = torch.cat([reb.symbols(ref.bottleneck_layer.encoder(xc[i:i + 16])) for i in range(0, n, 16)]).reshape(n, -1)
    out = {'what': 'encoder precisions alternated in one process: stage_front ms per batch per round; symbols of the first {} images '
                   'against the f32 CPU oracle encoder'.format(n), 'batch': args.batch, 'images_checked': n, 'rounds': args.rounds,
           'reps_per_interval': args.reps, 'device': torch.cuda.get_device_name(dev), 'modes': {}}
    hw = None
    with torch.no_grad():
        for mode in MODES:
            model.set_encoder_precision(mode)
            sym, hw = model.stage_front(x[:n])
            _, _, nb, st = eb.encode_symbols_device(sym, hw[0] * hw[1])
            assert int(st.max().item()) == 0
            diff = sym.cpu().reshape(n, -1) != ref_sym
            out['modes'][mode] = {'symbol_mismatch_rate': diff.float().mean().item(),
                                  'images_with_identical_symbols': int((~diff.any(dim=1)).sum().item()),
                                  'bpp': 8.0 * float(nb.sum().item()) / (n * pix), 'stage_front_ms_per_batch': []}
            model.stage_front(x)        # packs the weights, warms the allocator
        torch.cuda.synchronize(dev)
        for _ in range(args.rounds):
            for mode in MODES:
                model.set_encoder_precision(mode)
                model.stage_front(x)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    model.stage_front(x)
                e1.record()
                torch.cuda.synchronize(dev)
                out['modes'][mode]['stage_front_ms_per_batch'].append(round(e0.elapsed_time(e1) / args.reps, 4))
        if args.launches:
            for mode in MODES:
                model.set_encoder_precision(mode)
                torch.cuda.synchronize(dev)
                with hip.KernelTimer() as kt:
                    for _ in range(args.reps):
                        model.stage_front(x)
                    torch.cuda.synchronize(dev)
                out['modes'][mode]['launch_ms'] = {k: round(ms, 4) for k, (_, ms) in sorted(kt.summary().items())}
    model.set_encoder_precision('bf16')
    ref_len = sum(len(q) for q in bench.oracle_streams(ref, ref_sym, hw[0] * hw[1]))
    out['reference_f32_cpu_bpp'] = 8.0 * ref_len / (n * pix)
    f32 = out['modes']['f32']['stage_front_ms_per_batch']
    for mode in ('bf16x3', 'bf16x6'):
        t = out['modes'][mode]['stage_front_ms_per_batch']
        out['modes'][mode]['f32_over_this_per_round'] = [round(a / b, 3) for a, b in zip(f32, t)]
        out['modes'][mode]['faster_than_f32_in_every_round'] = all(b < a for a, b in zip(f32, t))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
