"""The four encoder precisions side by side on one box, in one process: the bench model at bs 256, 224 x 224.

    python tools/encoder_modes.py [--rounds 3] [--reps 5] [--launches] [--model fp | mshp | shp | factorized | hyperprior | mean]

The modes ('bf16', 'f32', 'bf16x3', 'bf16x6') are ALTERNATED for --rounds rounds, so that clock and thermal drift fall on all of
them alike.  Per mode: the `stage_front` time per batch of every round (HIP events, as bench.py's precision_check), the symbol
mismatch against the oracle's f32 CPU encoder on the first 64 images, the images whose symbols are all identical, and the bpp of
the streams the device codes from them.  --launches adds the per-launch times of one extra pass (hip.KernelTimer).
--model mshp | shp: the hyperprior bottlenecks instead (the mshp224 model of benchlib.workloads, or its scale-hyperprior twin),
where the mode is a property of the codec (g_a, h_a and h_s): `stage_front` ms per batch, and against the oracle's f32 CPU chain
the mismatch rates of z symbols, indexes and y symbols and the number of images with all three equal.
--model factorized | hyperprior | mean: the neural input compression models of compression.py (FactorizedPrior, ScaleHyperprior,
MeanScaleHyperprior at N = 128, M = 192, the operating point of tests/ref_split_input.py) on 128 x 192 images, where the mode covers
g_a, h_a, h_s and g_s: ms per batch of `stage_front` (factorized) or `compress` (the hyperprior models: both transforms, the hyper
transforms and the coders) and of `decompress`, and the same mismatch table against the oracle's f32 CPU chain on the first 8 images.
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


def _shp_twin(dev):
    """The scale-hyperprior twin of the mshp224 model: the same seed and operating point, the one-headed h_s tail scaled as a whole."""
    import sc2bench_amd as S
    torch.manual_seed(0)
    bl = S.get_layer('SHPBasedResNetBottleneck')
    with torch.no_grad():
        eb = bl.entropy_bottleneck
        q = torch.zeros(eb.channels, 1, 3)
        for c in range(eb.channels):
            q[c, 0, 0], q[c, 0, 1], q[c, 0, 2] = -(3 + c % 5), 0.25 * (c % 3), 4 + c % 7
        eb.quantiles.copy_(q)
        bl.g_a[4].weight.mul_(10.0)
        bl.h_a[2].weight.mul_(4.0)
        bl.h_s[4].weight.abs_().mul_(5.0)
    bl.eval().to(dev)
    bl.update()
    return bl


def main_hyper(args, dev):
    from benchlib.model import synthetic_batch
    from benchlib.workloads import build_workload
    from oracle import cpu_ref as R
    if args.model == 'mshp':
        bl = build_workload('mshp224', dev, args.batch)[0].bottleneck_layer
    else:
        bl = _shp_twin(dev)
    name = type(bl).__name__
    mshp = name.startswith('MSHP')
    x = synthetic_batch(args.batch, dev, seed=0)
    n = min(32, args.batch)
    ref = getattr(R, name)()
    own = ref.state_dict()
    ref.load_state_dict({k: v.detach().cpu() for k, v in bl.state_dict().items() if k in own and own[k].shape == v.shape}, strict=False)
    ref.eval()
    ref.update()
    xc = x[:n].float().cpu()
    with torch.no_grad():      # the oracle's f32 chain: what the reference's encode() computes before the coder
        y = ref.g_a(xc)
        z = ref.h_a(y if mshp else y.abs())
        z_hat = ref.entropy_bottleneck.quantize(z, 'dequantize', ref._get_means(z))
        params = ref.h_s(z_hat)
        scales, means = params.chunk(2, 1) if mshp else (params, None)
        want = (ref.entropy_bottleneck.symbols(z).int().reshape(n, -1), ref.gaussian_conditional.build_indexes(scales).int().reshape(n, -1),
                ref.gaussian_conditional.quantize(y, 'symbols', means).int().reshape(n, -1))
    out = {'what': '{}: codec precisions alternated in one process: stage_front ms per batch per round; z symbols, indexes and y symbols of '
                   'the first {} images against the oracle\'s f32 CPU chain'.format(name, n), 'model': args.model, 'batch': args.batch,
           'images_checked': n, 'rounds': args.rounds, 'reps_per_interval': args.reps, 'device': torch.cuda.get_device_name(dev), 'modes': {}}
    with torch.no_grad():
        for mode in MODES:
            bl.set_encoder_precision(mode)
            (y_sym, idx, z_sym), _ = bl.stage_front(x[:n])
            diff = [a.cpu().reshape(n, -1) != b for a, b in zip((z_sym, idx, y_sym), want)]
            same = ~(diff[0].any(dim=1) | diff[1].any(dim=1) | diff[2].any(dim=1))
            out['modes'][mode] = {'z_symbol_mismatch_rate': diff[0].float().mean().item(), 'index_mismatch_rate': diff[1].float().mean().item(),
                                  'y_symbol_mismatch_rate': diff[2].float().mean().item(),
                                  'images_with_all_three_identical': int(same.sum().item()), 'stage_front_ms_per_batch': []}
            bl.stage_front(x)        # packs the weights, warms the allocator
        torch.cuda.synchronize(dev)
        for _ in range(args.rounds):
            for mode in MODES:
                bl.set_encoder_precision(mode)
                bl.stage_front(x)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    bl.stage_front(x)
                e1.record()
                torch.cuda.synchronize(dev)
                out['modes'][mode]['stage_front_ms_per_batch'].append(round(e0.elapsed_time(e1) / args.reps, 4))
        if args.launches:
            for mode in MODES:
                bl.set_encoder_precision(mode)
                torch.cuda.synchronize(dev)
                with hip.KernelTimer() as kt:
                    for _ in range(args.reps):
                        bl.stage_front(x)
                    torch.cuda.synchronize(dev)
                out['modes'][mode]['launch_ms'] = {k: round(ms, 4) for k, (_, ms) in sorted(kt.summary().items())}
    bl.set_encoder_precision('bf16')
    print(json.dumps(out))


INPUT_MODELS = {'factorized': 'FactorizedPrior', 'hyperprior': 'ScaleHyperprior', 'mean': 'MeanScaleHyperprior'}


def _timed_rounds(fn, set_mode, args, dev):
    """ms per call of fn() per round, the modes alternated: -> {mode: [ms, ...]}"""
    ms = {mode: [] for mode in MODES}
    for _ in range(args.rounds):
        for mode in MODES:
            set_mode(mode)
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize(dev)
            ms[mode].append(round(e0.elapsed_time(e1) / args.reps, 4))
    return ms


def main_input(args, dev):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import ref_split_input as ri
    import sc2bench_amd as S
    name = INPUT_MODELS[args.model]
    ref = ri.build(name)
    m = S.COMPRESSION_MODEL_CLASS_DICT[name](ri.N_CH, ri.M_CH)
    m.load_state_dict({k: v.clone() for k, v in ref.state_dict().items()})
    m.eval().to(dev)
    hyper = ri.has_hyper(ref)
    n = min(8, args.batch)
    xc = torch.rand(args.batch, 3, 128, 192, generator=torch.Generator().manual_seed(1234))
    x = xc.to(dev)
    want = [t.reshape(n, -1) for t in ri.int_tensors(ri.stages(ref, xc[:n], 'f32'))]
    front = 'compress' if hyper else 'stage_front'
    out = {'what': '{}: codec precisions alternated in one process: {} and decompress ms per batch per round; the integer tensors of the '
                   'first {} images against the oracle\'s f32 CPU chain'.format(name, front, n), 'model': args.model, 'batch': args.batch,
           'image': [128, 192], 'images_checked': n, 'rounds': args.rounds, 'reps_per_interval': args.reps,
           'device': torch.cuda.get_device_name(dev), 'modes': {}}
    enc = {}
    with torch.no_grad():
        for mode in MODES:
            m.set_encoder_precision(mode)
            y = m.analysis(x[:n])
            if hyper:
                gc = m.gaussian_conditional
                e = m.compress(x[:n])
                scales, means = m._gaussian(m.hyper_synthesis(m._z_hat_nhwc(e['strings'][1], e['shape'])))
                got = (m.entropy_bottleneck.symbols_device(m.hyper_analysis(y)), gc.build_indexes(scales), gc.quantize(y, 'symbols', means))
                names = ('z_symbol', 'index', 'y_symbol')
            else:
                got, names = (m.entropy_bottleneck.symbols_device(y),), ('y_symbol',)
            diff = [a.cpu().int().reshape(n, -1) != b for a, b in zip(got, want)]
            same = ~torch.stack([d.any(dim=1) for d in diff]).any(dim=0)
            out['modes'][mode] = {'{}_mismatch_rate'.format(k): d.float().mean().item() for k, d in zip(names, diff)}
            out['modes'][mode]['images_with_all_identical'] = int(same.sum().item())
            enc[mode] = m.compress(x)          # packs the weights, warms the allocator; decompress decodes its own mode's streams
            m.decompress(**enc[mode])
        torch.cuda.synchronize(dev)
        mode_now = []

        def set_mode(mode):
            m.set_encoder_precision(mode)
            mode_now[:] = [mode]

        for key, fn in (('{}_ms_per_batch'.format(front), (lambda: m.compress(x)) if hyper else (lambda: m.stage_front(x))),
                        ('decompress_ms_per_batch', lambda: m.decompress(**enc[mode_now[0]]))):
            for mode, ms in _timed_rounds(fn, set_mode, args, dev).items():
                out['modes'][mode][key] = ms
        if args.launches:
            for mode in MODES:
                set_mode(mode)
                torch.cuda.synchronize(dev)
                with hip.KernelTimer() as kt:
                    m.decompress(**m.compress(x))
                    torch.cuda.synchronize(dev)
                out['modes'][mode]['launch_ms'] = {k: round(ms, 4) for k, (_, ms) in sorted(kt.summary().items())}
    m.set_encoder_precision('bf16')
    for key in ('{}_ms_per_batch'.format(front), 'decompress_ms_per_batch'):
        base = out['modes']['bf16'][key]
        for mode in MODES[1:]:
            out['modes'][mode][key.replace('_ms_per_batch', '_over_bf16_per_round')] = [round(a / b, 3) for a, b in zip(out['modes'][mode][key], base)]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5, help='stage_front calls per timed interval')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--model', choices=('fp', 'mshp', 'shp') + tuple(INPUT_MODELS), default='fp',
                    help='fp: the bench model (default); mshp / shp: the hyperprior bottlenecks; factorized / hyperprior / mean: the input codecs')
    args = ap.parse_args()
    assert args.rounds >= 3
    dev = torch.device('cuda:0')
    if args.model in INPUT_MODELS:
        return main_input(args, dev)
    if args.model != 'fp':
        return main_hyper(args, dev)
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
