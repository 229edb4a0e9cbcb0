"""-m gpu: the F32 form of the context-model scan (sc2_ar_scan_f32 of csrc/ar_context.hip: the same step with the four weight
matrices read as f32), called directly and held to the sequential reference of tests/ref_ar_scan.py on the operand sets of
tests/ref_ar_scan_f32.py (checked on the CPU in tests/test_ar_scan_f32_ref_cpu.py).

The conventions are those of tests/test_gpu_ar_scan.py, whose helpers are used as they are: every operand and output between
guard bands, the decoder's streams CPU-encoded with the oracle coder at non-zero offsets inside filled rows.
- the exact sets of the bf16 test, uploaded as f32: bit for bit (the shared step code still is the step);
- (a) f32-only Gaussian weights: within the running f32 bound of the float64 step ON THOSE WEIGHTS -- a scan that rounded them to
  bf16 leaves that bound by a factor of 10 to 950 (the CPU test), so this cannot pass on the bf16 kernel;
- (b) four cases that turn on the low bits of one weight of one matrix each: bit for bit, symbols off by one otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exact_ints as EI  # noqa: E402
import ref_ar_scan as RA  # noqa: E402
import ref_ar_scan_f32 as RF  # noqa: E402
import test_gpu_ar_scan as T  # noqa: E402  (helpers only: pytest collects a module's tests where it finds the file, not here)

BASE = RA.SMALL_SHAPES[0]
_id = T._id


def _case(kind, key):
    """-> (case, float64 reference, how often the images repeat); kinds: 'exact' (the bf16 test's set), 'random_f32', 'lowbits'."""
    if kind == 'exact':
        return T._case('exact', key)
    return RF.cached(kind, key) + (1,)


_OPS = {}


def _ops(kind, key, dev):
    k = (kind, tuple(key) if kind != 'lowbits' else key)
    if k not in _OPS:
        case, _, rep = _case(kind, key)
        w = {n: EI.arena(torch.from_numpy(np.ascontiguousarray(v)).float(), device=dev) for n, v in case['weights'].items()}
        for n, v in case['weights'].items():
            assert w[n].dtype == torch.float32 and np.array_equal(w[n].cpu().double().numpy(), v), n   # the upload rounded nothing
        M, _, _, H, W, _ = case['shape']
        _OPS[k] = {'w': w, 'p1': EI.arena(torch.from_numpy(T._tiled(case['p1'], rep)).float(), device=dev),
                   'y': EI.arena(torch.from_numpy(T._tiled(case['y'], rep)).float(), device=dev),
                   'table': EI.arena(torch.from_numpy(case['scale_table']).float(), device=dev),
                   'bound': case['scale_bound'], 'dims': (case['p1'].shape[0] * rep, M, H, W)}
    return _OPS[k]


def _encode(S, dev, kind, key, ranges=None, pad_fill=0.0):
    ops = _ops(kind, key, dev)
    o = T._outputs(ops, dev, pad_fill)
    for pix in ranges or [None]:
        S.hip.ar_scan(ops['w'], ops['p1'], o['y_hat_pad'], o['y_hat_nhwc'], ops['table'], ops['bound'], y=ops['y'],
                      symbols=o['symbols'], indexes=o['indexes'], pix=pix, gaussian_params=o['gaussian_params'])
    return T._finish(ops, o)


_ENC = {}


def _encoded(S, dev, kind, key):
    k = (kind, tuple(key) if kind != 'lowbits' else key)
    if k not in _ENC:
        _ENC[k] = _encode(S, dev, kind, key)
    return _ENC[k]


# --------------------------------------------------------------------------------------------- #
# encoder
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('shape', T.EXACT_SHAPES, ids=_id)
def test_exact_set_as_f32_is_bit_equal_to_the_reference(S, dev, shape):
    _, ref, rep = _case('exact', shape)
    got = _encoded(S, dev, 'exact', shape)
    RA.assert_exact(got, {k: T._tiled(v, rep) for k, v in ref.items()})


@pytest.mark.parametrize('shape', RA.SMALL_SHAPES, ids=_id)
def test_f32_weights_within_the_running_bound(S, dev, shape):
    case, _, _ = _case('random_f32', shape)
    got = _encoded(S, dev, 'random_f32', shape)
    ratio = RA.assert_random(case, got)
    print('ar_scan f32 random set {}: largest |err| / bound = {:.4g}'.format(_id(shape), ratio))
    assert ratio < 1


@pytest.mark.parametrize('matrix', RF.MATRICES)
def test_low_bits_of_one_weight_reach_the_symbols(S, dev, matrix):
    case, ref, _ = _case('lowbits', matrix)
    got = _encoded(S, dev, 'lowbits', matrix)
    RA.assert_exact(got, ref)
    assert np.array_equal(got['symbols'].reshape(case['symbols'].shape), case['symbols'])
    assert not np.array_equal(got['symbols'].reshape(case['symbols'].shape), case['symbols_bf16'])


@pytest.mark.parametrize('kind', ['exact', 'random_f32'])
def test_pixels_not_yet_reached_are_never_read(S, dev, kind):
    """NaN in the whole interior of y_hat_pad before the scan (the border stays zero): the same bits as from zeros."""
    T._assert_same(_encode(S, dev, kind, BASE, pad_fill=float('nan')), _encoded(S, dev, kind, BASE))


@pytest.mark.parametrize('kind', ['exact', 'random_f32'])
def test_encoder_split_into_pixel_ranges(S, dev, kind):
    T._assert_same(_encode(S, dev, kind, BASE, ranges=T._ranges(BASE)), _encoded(S, dev, kind, BASE))


# --------------------------------------------------------------------------------------------- #
# decoder
# --------------------------------------------------------------------------------------------- #
def _tables(kind, dev):
    """The CDF tables depend on the scale table alone: (a) shares the bf16 random set's."""
    if kind == 'random_f32':
        assert np.array_equal(RF.cached(kind, BASE)[0]['scale_table'], RA.cached('random', BASE)[0]['scale_table'])
    return T._tables('exact' if kind == 'exact' else 'random', dev)


def _decode(S, dev, kind, shape, packed, ranges=None):
    ops = _ops(kind, shape, dev)
    B = ops['dims'][0]
    o = T._outputs(ops, dev)
    state = {'st_x': EI.arena_like((B,), torch.int64, dev), 'st_pos': EI.arena_like((B,), torch.int32, dev),
             'status': EI.arena_like((B,), torch.int32, dev)}
    dec = dict(_tables(kind, dev)[1], **state)
    for name, a in zip(('buf', 'off', 'nb'), packed):
        dec[name] = EI.arena(torch.from_numpy(a), device=dev)
    for pix in ranges or [None]:
        S.hip.ar_scan(ops['w'], ops['p1'], o['y_hat_pad'], o['y_hat_nhwc'], ops['table'], ops['bound'], symbols=o['symbols'],
                      indexes=o['indexes'], decode=dec, pix=pix, gaussian_params=o['gaussian_params'])
    out = T._finish(ops, o, extra=list(state.items()))
    return out, {k: v.cpu().numpy() for k, v in state.items()}


@pytest.mark.parametrize('kind,shape', [('exact', s) for s in RA.SMALL_SHAPES] + [('random_f32', s) for s in RA.SMALL_SHAPES],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_decoder_returns_the_encoder_run(S, dev, kind, shape):
    """As in the bf16 test: the exact set's CDF rows alone exceed the 160 KiB of LDS (searched in device memory), the random
    set's fit beside the largest step vectors (kept in LDS); the LDS layout does not depend on the weight type."""
    entries = _tables(kind, dev)[1]['cdf_entries']
    M, C1p, C2p = shape[:3]
    step_words = 12 * M + 4 * M + C1p + C2p + 4 * max(2 * M, C1p, C2p) + 2 * M + 4 * len(_case(kind, shape)[0]['scale_table'])
    if kind == 'exact':
        assert 2 * entries > 160 * 1024
    else:
        assert 4 * step_words + 2 * entries + 2 <= 160 * 1024
    enc = _encoded(S, dev, kind, shape)
    strings = T._strings(enc, _tables(kind, dev)[0])
    out, state = _decode(S, dev, kind, shape, T._pack(strings, 0xFF))
    T._assert_same(out, enc)
    assert not state['status'].any(), state['status']


@pytest.mark.parametrize('kind', ['exact', 'random_f32'])
def test_decoder_split_into_pixel_ranges(S, dev, kind):
    enc = _encoded(S, dev, kind, BASE)
    packed = T._pack(T._strings(enc, _tables(kind, dev)[0]), 0xFF)
    whole, st_whole = _decode(S, dev, kind, BASE, packed)
    split, st_split = _decode(S, dev, kind, BASE, packed, ranges=T._ranges(BASE))
    T._assert_same(split, enc)
    T._assert_same(whole, enc)
    T._assert_same(st_split, st_whole)
    assert not st_split['status'].any()


# --------------------------------------------------------------------------------------------- #
# routing
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('odd', RF.MATRICES)
def test_mixed_weight_dtypes_are_refused_before_launch(S, dev, odd):
    ops = _ops('random_f32', BASE, dev)
    o = T._outputs(ops, dev)
    for base, other in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
        w = {k: (v.to(other if k == odd else base) if k in RF.MATRICES else v) for k, v in ops['w'].items()}
        with pytest.raises(S.hip.Sc2Error, match='all bf16 or all f32'):
            S.hip.ar_scan(w, ops['p1'], o['y_hat_pad'], o['y_hat_nhwc'], ops['table'], ops['bound'], y=ops['y'],
                          symbols=o['symbols'], indexes=o['indexes'], gaussian_params=o['gaussian_params'])
    torch.cuda.synchronize()
    for name, t in o.items():                 # nothing ran: every output still holds its fill, the interior of y_hat_pad its zeros
        EI.assert_bands_untouched(t, name)
    assert int((o['symbols'] != EI.INT_SENTINEL[torch.int32]).sum()) == 0
    assert torch.isnan(o['gaussian_params']).all() and not o['y_hat_pad'].any()
