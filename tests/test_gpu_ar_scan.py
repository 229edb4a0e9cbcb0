"""-m gpu: the context-model scan kernels of csrc/ar_context.hip (sc2_ar_scan, sc2_rans_decode_resume) called directly and held
to the sequential reference of tests/ref_ar_scan.py (itself checked on the CPU in tests/test_ar_scan_ref_cpu.py).

Exact set: every sum is an exact f32 number in any order, so symbols, indexes, gaussian params and y_hat equal the float64
reference bit for bit.  Random set: gaussian params within the derived f32 bound of their float64 value given the kernel's own
y_hat, everything downstream of them exactly.  Every operand and output lives between guard bands (exact_ints.arena); the
decoder's streams are CPU-encoded with the oracle coder and sit at non-zero offsets inside rows whose padding is filled."""
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

ST_INDEX, ST_CORRUPT, ST_TAIL = 4, 8, 16          # status bits 2, 3, 4
EXACT_SHAPES = RA.SMALL_SHAPES + RA.WIDE_SHAPES + [RA.MANY_IMAGES]
BASE = RA.SMALL_SHAPES[0]


def _id(shape):
    return 'x'.join(str(v) for v in shape)


# --------------------------------------------------------------------------------------------- #
# operands, outputs, launches
# --------------------------------------------------------------------------------------------- #
def _case(kind, shape):
    """-> (case, reference, how often the images repeat): the many-images case is three images tiled."""
    if tuple(shape) == RA.MANY_IMAGES:
        case, ref = RA.cached(kind, shape[:5] + (RA.MANY_DISTINCT,))
        return case, ref, shape[5] // RA.MANY_DISTINCT
    return RA.cached(kind, shape) + (1,)


def _tiled(a, rep):
    return np.tile(a, (rep,) + (1,) * (a.ndim - 1)) if rep > 1 else a


_OPS = {}


def _ops(kind, shape, dev):
    key = (kind, tuple(shape))
    if key not in _OPS:
        case, _, rep = _case(kind, shape)
        w = {k: EI.arena(torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16 if k[0] == 'w' else torch.float32), device=dev)
             for k, v in case['weights'].items()}
        for k, v in case['weights'].items():
            assert np.array_equal(w[k].cpu().double().numpy(), v), k          # the upload rounded nothing
        M, _, _, H, W, _ = case['shape']
        _OPS[key] = {'w': w, 'p1': EI.arena(torch.from_numpy(_tiled(case['p1'], rep)).float(), device=dev),
                     'y': EI.arena(torch.from_numpy(_tiled(case['y'], rep)).float(), device=dev),
                     'table': EI.arena(torch.from_numpy(case['scale_table']).float(), device=dev),
                     'bound': case['scale_bound'], 'dims': (case['p1'].shape[0] * rep, M, H, W)}
    return _OPS[key]


def _outputs(ops, dev, pad_fill=0.0):
    B, M, H, W = ops['dims']
    pad = torch.zeros((B, H + 2, W + 4, M))
    pad[:, 2:, 2:W + 2, :] = pad_fill
    return {'y_hat_pad': EI.arena(pad, device=dev), 'y_hat_nhwc': EI.arena_like((B, H, W, M), torch.bfloat16, dev),
            'symbols': EI.arena_like((B, H * W * M), torch.int32, dev), 'indexes': EI.arena_like((B, H * W * M), torch.int32, dev),
            'gaussian_params': EI.arena_like((B, H * W, 2 * M), torch.float32, dev)}


def _finish(ops, o, extra=()):
    """Guard bands of everything the scan may write, y_hat_pad's zero border, then the outputs on the host."""
    torch.cuda.synchronize()
    W = ops['dims'][3]
    for name, t in list(o.items()) + list(extra):
        EI.assert_bands_untouched(t, name)
    pad = o['y_hat_pad']
    for name, part in (('rows above', pad[:, :2]), ('columns left', pad[:, :, :2]), ('columns right', pad[:, :, W + 2:])):
        assert int((part.contiguous().view(torch.int32) != 0).sum()) == 0, 'y_hat_pad: the zero border was written ({})'.format(name)
    out = {k: v.cpu() for k, v in o.items()}
    once = out['y_hat_pad'][:, 2:, 2:W + 2, :].to(torch.bfloat16)
    assert torch.equal(out['y_hat_nhwc'].view(torch.int16), once.contiguous().view(torch.int16)), \
        'y_hat_nhwc is not the bf16 of y_hat_pad, rounded once'
    return {k: (v.view(torch.int16) if v.dtype == torch.bfloat16 else v).numpy() for k, v in out.items()}


def _encode(S, dev, kind, shape, ranges=None, pad_fill=0.0):
    ops = _ops(kind, shape, dev)
    o = _outputs(ops, dev, pad_fill)
    for pix in ranges or [None]:
        S.hip.ar_scan(ops['w'], ops['p1'], o['y_hat_pad'], o['y_hat_nhwc'], ops['table'], ops['bound'], y=ops['y'],
                      symbols=o['symbols'], indexes=o['indexes'], pix=pix, gaussian_params=o['gaussian_params'])
    return _finish(ops, o)


_ENC = {}


def _encoded(S, dev, kind, shape):
    """The one-launch encoder run of a case, computed once and shared (read-only)."""
    key = (kind, tuple(shape))
    if key not in _ENC:
        _ENC[key] = _encode(S, dev, kind, shape)
    return _ENC[key]


def _assert_same(got, want, names=None):
    for name in names or want:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.dtype('u{}'.format(g.itemsize))) != w.view(np.dtype('u{}'.format(w.itemsize))))
            raise AssertionError('{}: {} of {} elements differ, first at {}'.format(name, len(bad), g.size, tuple(bad[0])))


# --------------------------------------------------------------------------------------------- #
# encoder
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=_id)
def test_exact_set_is_bit_equal_to_the_reference(S, dev, shape):
    _, ref, rep = _case('exact', shape)
    got = _encoded(S, dev, 'exact', shape)
    RA.assert_exact(got, {k: _tiled(v, rep) for k, v in ref.items()})


@pytest.mark.parametrize('shape', RA.SMALL_SHAPES, ids=_id)
def test_random_set_within_the_running_bound(S, dev, shape):
    case, _, _ = _case('random', shape)
    got = _encoded(S, dev, 'random', shape)
    ratio = RA.assert_random(case, got)
    print('ar_scan random set {}: largest |err| / bound = {:.4g}'.format(_id(shape), ratio))
    assert ratio < 1


@pytest.mark.parametrize('kind', ['exact', 'random'])
def test_pixels_not_yet_reached_are_never_read(S, dev, kind):
    """NaN in the whole interior of y_hat_pad before the scan (the border stays zero): the same bits as from zeros."""
    _assert_same(_encode(S, dev, kind, BASE, pad_fill=float('nan')), _encoded(S, dev, kind, BASE))


def _ranges(shape):
    H, W = shape[3], shape[4]
    assert W + 2 < H * W
    return [(0, 1), (1, 1), (1, W + 2), (W + 2, H * W)]


@pytest.mark.parametrize('kind', ['exact', 'random'])
def test_encoder_split_into_pixel_ranges(S, dev, kind):
    _assert_same(_encode(S, dev, kind, BASE, ranges=_ranges(BASE)), _encoded(S, dev, kind, BASE))


# --------------------------------------------------------------------------------------------- #
# decoder
# --------------------------------------------------------------------------------------------- #
_TABLES = {}


def _tables(kind, dev):
    """CDF tables of a GaussianConditional updated with the set's scale table: (host cdfs / sizes / offsets, device dict)."""
    if kind not in _TABLES:
        from oracle.cpu_ref import GaussianConditional
        gc = GaussianConditional(None)
        gc.update_scale_table(RA.cached(kind, BASE)[0]['scale_table'].tolist())
        host = (gc._quantized_cdf.int().numpy(), gc._cdf_length.reshape(-1).int().numpy(), gc._offset.reshape(-1).int().numpy())
        device = {'cdfs': EI.arena(torch.from_numpy(host[0]), device=dev), 'cdf_sizes': EI.arena(torch.from_numpy(host[1]), device=dev),
                  'offsets': EI.arena(torch.from_numpy(host[2]), device=dev), 'cdf_entries': int(host[1].sum()) - len(host[1])}
        _TABLES[kind] = (host, device)
    return _TABLES[kind]


def _strings(enc, host_tables):
    from oracle import rans as oracle_rans
    return [oracle_rans.encode_with_indexes(s, i, *host_tables) for s, i in zip(enc['symbols'], enc['indexes'])]


def _pack(strings, fill, offsets=None, nbytes=None):
    """Rows of one stream each, stream i at a non-zero offset that is a multiple of 4, every other byte of the row = `fill`."""
    n = len(strings)
    off = np.array([4 * (1 + i % 3) for i in range(n)] if offsets is None else offsets, dtype=np.int32)
    stride = (max(int(o) + len(s) for o, s in zip(off, strings)) + 3) // 4 * 4 + 16
    buf = np.full((n, stride), fill, dtype=np.uint8)
    for i, s in enumerate(strings):
        buf[i, off[i]:off[i] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    nb = np.array([len(s) for s in strings] if nbytes is None else nbytes, dtype=np.int32)
    return buf, off, nb


def _decode(S, dev, kind, shape, packed, ranges=None):
    """-> (outputs, state): the decoder scan over `packed` = (buf, off, nb); the state starts as sentinels, not zeros."""
    ops = _ops(kind, shape, dev)
    B = ops['dims'][0]
    o = _outputs(ops, dev)
    state = {'st_x': EI.arena_like((B,), torch.int64, dev), 'st_pos': EI.arena_like((B,), torch.int32, dev),
             'status': EI.arena_like((B,), torch.int32, dev)}
    dec = dict(_tables(kind, dev)[1], **state)
    for name, a in zip(('buf', 'off', 'nb'), packed):
        dec[name] = EI.arena(torch.from_numpy(a), device=dev)
    for pix in ranges or [None]:
        S.hip.ar_scan(ops['w'], ops['p1'], o['y_hat_pad'], o['y_hat_nhwc'], ops['table'], ops['bound'], symbols=o['symbols'],
                      indexes=o['indexes'], decode=dec, pix=pix, gaussian_params=o['gaussian_params'])
    out = _finish(ops, o, extra=list(state.items()))
    return out, {k: v.cpu().numpy() for k, v in state.items()}


@pytest.mark.parametrize('kind,shape', [('exact', s) for s in RA.SMALL_SHAPES] + [('random', s) for s in RA.SMALL_SHAPES],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_decoder_returns_the_encoder_run(S, dev, kind, shape):
    """The exact set's symbols in the hundreds are mostly escapes.  Its CDF rows (scales up to 4096) alone exceed the 160 KiB of
    LDS, so the library has to search them in device memory, and the random set's rows fit beside the largest step vectors,
    so it may keep them in LDS: the sizes are asserted here, which variant the library launched is not observable from
    outside and is not asserted."""
    entries = _tables(kind, dev)[1]['cdf_entries']
    M, C1p, C2p = shape[:3]
    step_words = 12 * M + 4 * M + C1p + C2p + 4 * max(2 * M, C1p, C2p) + 2 * M + 4 * len(RA.cached(kind, shape)[0]['scale_table'])
    if kind == 'exact':
        assert 2 * entries > 160 * 1024
    else:
        assert 4 * step_words + 2 * entries + 2 <= 160 * 1024
    enc = _encoded(S, dev, kind, shape)
    strings = _strings(enc, _tables(kind, dev)[0])
    out, state = _decode(S, dev, kind, shape, _pack(strings, 0xFF))
    _assert_same(out, enc)
    assert not state['status'].any(), state['status']


@pytest.mark.parametrize('kind', ['exact', 'random'])
def test_decoder_split_into_pixel_ranges(S, dev, kind):
    enc = _encoded(S, dev, kind, BASE)
    packed = _pack(_strings(enc, _tables(kind, dev)[0]), 0xFF)
    whole, st_whole = _decode(S, dev, kind, BASE, packed)
    split, st_split = _decode(S, dev, kind, BASE, packed, ranges=_ranges(BASE))
    _assert_same(split, enc)
    _assert_same(whole, enc)
    _assert_same(st_split, st_whole)
    assert not st_split['status'].any()


def _both_fills(S, dev, kind, strings, **kw):
    """The same decode with 0x00 and with 0xFF in every byte of the rows outside the streams: nothing may depend on them."""
    runs = [_decode(S, dev, kind, BASE, _pack(strings, fill, **kw)) for fill in (0x00, 0xFF)]
    _assert_same(runs[1][0], runs[0][0], names=['symbols'])
    _assert_same(runs[1][1], runs[0][1])
    return runs[0]


@pytest.mark.parametrize('kind', ['exact', 'random'])
def test_no_byte_outside_a_stream_is_read(S, dev, kind):
    enc = _encoded(S, dev, kind, BASE)
    strings = _strings(enc, _tables(kind, dev)[0])
    assert len(strings) >= 2 and all(len(s) % 4 == 0 and len(s) >= 16 for s in strings)
    out, state = _both_fills(S, dev, kind, strings)
    _assert_same(out, enc, names=['symbols', 'indexes', 'y_hat_pad'])
    assert not state['status'].any()
    # stream 0 cut to half its length: zeros are supplied past its end, whatever the row holds there
    half = len(strings[0]) // 2 // 4 * 4
    out, state = _both_fills(S, dev, kind, [strings[0][:half], strings[1]])
    assert state['status'][0] & ST_CORRUPT and state['status'][1] == 0, state['status']
    n = out['symbols'].shape[1]
    assert np.array_equal(out['symbols'][1], enc['symbols'][1])
    assert not np.array_equal(out['symbols'][0], enc['symbols'][0]) and n == enc['symbols'].shape[1]


@pytest.mark.parametrize('kind', ['exact', 'random'])
def test_flagged_stream_layouts(S, dev, kind):
    enc = _encoded(S, dev, kind, BASE)
    strings = _strings(enc, _tables(kind, dev)[0])
    # an offset of 2 inside the row
    out, state = _both_fills(S, dev, kind, strings, offsets=[2, 8])
    assert state['status'][0] & ST_CORRUPT and state['status'][1] == 0, state['status']
    assert np.array_equal(out['symbols'][1], enc['symbols'][1])
    # a length that overruns the row, on a stream that is not the last
    buf, off, nb = _pack(strings, 0xFF)
    over = [buf.shape[1] - int(off[0]) + 4, int(nb[1])]
    out, state = _both_fills(S, dev, kind, strings, nbytes=over)
    assert state['status'][0] & ST_CORRUPT and state['status'][1] == 0, state['status']
    assert np.array_equal(out['symbols'][1], enc['symbols'][1])
    # four more bytes than the encoder wrote: every symbol is right and the stream does not end where the last pixel does
    out, state = _both_fills(S, dev, kind, [strings[0] + b'\x00\x00\x00\x00', strings[1]])
    assert state['status'][0] == ST_TAIL and state['status'][1] == 0, state['status']
    _assert_same(out, enc, names=['symbols', 'indexes', 'y_hat_pad'])


# --------------------------------------------------------------------------------------------- #
# the resumable decoder
# --------------------------------------------------------------------------------------------- #
N_STREAMS, N_SYM = 130, 300           # three blocks of 64 streams, the last one partial
CUTS = [0, 0, 1, 150, 300]            # the first call is empty


def _resume_inputs(dev):
    from oracle import rans as oracle_rans
    host, device = _tables('random', dev)
    g = torch.Generator().manual_seed(4)
    idx = torch.randint(0, host[0].shape[0], (N_STREAMS, N_SYM), generator=g, dtype=torch.int32)
    idx[70, 5] = 7                             # not row 0: the row decoded in place of a bad index there is the wrong one
    sym = (torch.randn(N_STREAMS, N_SYM, generator=g) * (idx.float() + 1) * 2).round().int()
    sym[3, :40] = 100000                       # escapes
    sym[129, -5:] = -70000
    sym[70, 5] = 0                             # inside row 7 (an escape would leave the same state under either row)
    strings = [oracle_rans.encode_with_indexes(sym[i].numpy(), idx[i].numpy(), *host) for i in range(N_STREAMS)]
    buf, off, nb = (EI.arena(torch.from_numpy(a), device=dev) for a in _pack(strings, 0xFF))
    return sym, idx, (buf, off, nb), device


def _resume(S, dev, packed, idx, tables, cuts):
    idx_d = idx.to(dev)
    state, parts = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s, state = S.hip.rans_decode_resume(packed[0], packed[1], packed[2], idx_d[:, a:b].contiguous(), tables['cdfs'],
                                            tables['cdf_sizes'], tables['offsets'], state=state, last=b == cuts[-1] and b > a)
        parts.append(s)
    torch.cuda.synchronize()
    EI.assert_bands_untouched(packed[0], 'streams')
    return torch.cat(parts, 1).cpu(), state[2].cpu()


def test_resumable_decoder_over_three_blocks(S, dev):
    sym, idx, packed, tables = _resume_inputs(dev)
    got, status = _resume(S, dev, packed, idx, tables, CUTS)
    assert torch.equal(got, sym)
    assert not status.any(), status.nonzero().reshape(-1)
    # one index outside the table, in the second call that decodes anything: flagged on that stream alone, through to the end
    bad = idx.clone()
    bad[70, 5] = tables['cdfs'].shape[0]
    for cuts in (CUTS, [0, N_SYM]):
        got, status = _resume(S, dev, packed, bad, tables, cuts)
        assert int(status[70]) & ST_INDEX, (cuts, int(status[70]))
        others = torch.arange(N_STREAMS) != 70
        assert not status[others].any(), status.nonzero().reshape(-1)
        assert torch.equal(got[others], sym[others])
        assert torch.equal(got[70, :5], sym[70, :5])
        assert not torch.equal(got[70, 6:], sym[70, 6:])       # the stream did lose step, and bit 2 outlived what followed
