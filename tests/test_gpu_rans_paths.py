"""Every decode-side kernel of csrc/rans.hip on the device, case by case of tests/ref_rans_paths.py (which says which case launches
which kernel and why; tests/test_rans_paths_ref_cpu.py holds the case table to the oracle).  Per case, under the case's policy:

  * the library reports the decoder the restated dispatch expects (hip.rans_decode_path == ref.plan);
  * the device encoder's bytes are the oracle's for every stream, and the decoders are fed the ORACLE's bytes;
  * one call through the hip.* wrapper and one through the C entry point, there with every output (symbols_out, status, y_hat, the
    workspace) inside a sentinel-filled arena of exactly its extent: guards intact, every element of symbols_out, status and
    y_hat written, the two calls bit-equal;
  * status 0, symbols == the case's, y_hat == ref.dequantize_ref bit for bit (and == hip.eb_dequantize of the symbols), the fused call
    with symbols_out == the one without.

No tolerance anywhere: symbols, status words and bf16 bits are compared for equality."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import ref_rans_paths as ref

pytestmark = pytest.mark.gpu

POLICY_FIELDS = tuple(ref.DEFAULT_POLICY)
I16, I32 = torch.int16, torch.int32


@contextlib.contextmanager
def _policy(hip, overrides):
    """the case's policy, and afterwards whatever get_policy() returned before"""
    before = hip.get_policy()
    saved = {f: getattr(before, f) for f in POLICY_FIELDS}
    assert saved == ref.DEFAULT_POLICY, saved          # (tests start from the library's defaults, which ref.plan restates)
    try:
        if overrides:
            hip.configure(**overrides)
        yield
    finally:
        hip.configure(**saved)


class _Arena(object):
    """`n` int16 / int32 elements between two bands of PAD sentinel elements (the style of tests/test_gpu_stream_kernels.py)"""
    PAD = 4096

    def __init__(self, n, dtype, dev):
        self.n, self.sentinel = n, 0x5A5A if dtype == I16 else 0x5A5A5A5A
        self.buf = torch.full((n + 2 * self.PAD,), self.sentinel, dtype=dtype, device=dev)
        assert self.buf.data_ptr() % 16 == 0

    def payload(self):
        return self.buf[self.PAD:self.PAD + self.n]

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.PAD * self.buf.element_size())

    def guards_intact(self):
        return bool((self.buf[:self.PAD] == self.sentinel).all()) and bool((self.buf[self.PAD + self.n:] == self.sentinel).all())

    def all_written(self):
        return not bool((self.payload() == self.sentinel).any())

    def untouched(self):
        return bool((self.buf == self.sentinel).all())


def _device(dev, c, b, streams=None):
    buf, off, nb = ref.pack_streams(b.streams if streams is None else streams)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return {'buf': t(buf), 'off': t(off), 'nb': t(nb), 'cdfs': t(b.cdfs), 'sizes': t(b.sizes), 'offs': t(b.offs), 'sym': t(b.sym),
            'idx': t(b.idx) if c.explicit else None, 'med': t(b.medians) if c.fused else None}


def _c_call(hip, dev, c, d, want_symbols=True):
    """the decode through the C entry point, outputs in arenas -> (symbols or None, status, y_hat or None); guards and coverage checked"""
    lib, p = hip.lib(), hip._ptr
    n_cdfs, stride = d['cdfs'].shape
    ws_bytes = int(lib.sc2_rans_workspace_bytes(c.S, c.n_sym, n_cdfs, stride))
    assert ws_bytes % 4 == 0
    a_sym = _Arena(c.S * c.n_sym, I32, dev)
    a_st = _Arena(c.S, I32, dev)
    a_ws = _Arena(ws_bytes // 4, I32, dev)
    a_y = _Arena(c.S * c.HW * c.C, I16, dev) if c.fused else None
    if c.fused:
        rc = lib.sc2_rans_decode_dequantize_batch(p(d['buf']), d['buf'].shape[1], p(d['off']), p(d['nb']), c.index_div, c.S, c.n_sym, p(d['cdfs']),
                                                  n_cdfs, stride, p(d['sizes']), p(d['offs']), p(d['med']), a_sym.ptr() if want_symbols else None,
                                                  a_y.ptr(), a_st.ptr(), a_ws.ptr(), ws_bytes, hip._stream())
    else:
        rc = lib.sc2_rans_decode_batch(p(d['buf']), d['buf'].shape[1], p(d['off']), p(d['nb']), p(d['idx']), c.index_div, c.S, c.n_sym, p(d['cdfs']),
                                       n_cdfs, stride, p(d['sizes']), p(d['offs']), a_sym.ptr(), a_st.ptr(), a_ws.ptr(), ws_bytes, hip._stream())
    assert rc == 0, (c.name, rc, lib.sc2_last_error())
    torch.cuda.synchronize()
    for what, a in (('symbols_out', a_sym), ('status', a_st), ('workspace', a_ws), ('y_hat', a_y)):
        if a is not None:
            assert a.guards_intact(), '{}: a write outside {}'.format(c.name, what)
    if want_symbols:
        assert a_sym.all_written(), '{}: an element of symbols_out was left unwritten'.format(c.name)
    else:
        assert a_sym.untouched(), c.name
    assert a_st.all_written(), '{}: an element of status was left unwritten'.format(c.name)
    if c.fused:
        assert a_y.all_written(), '{}: an element of y_hat was left unwritten'.format(c.name)
    return (a_sym.payload().reshape(c.S, c.n_sym) if want_symbols else None, a_st.payload(),
            a_y.payload().reshape(c.S, c.HW, c.C) if c.fused else None)


def _bytes_of(buf, off, nb):
    return ref.unpack_streams(buf.cpu().numpy(), off.cpu().numpy(), nb.cpu().numpy())


@pytest.mark.parametrize('name', [c.name for c in ref.CASES])
def test_decoder_path_is_exact(S, dev, name):
    hip = S.hip
    c = ref.CASE_BY_NAME[name]
    n_cdfs, stride = ref.case_shape(c)
    with _policy(hip, c.policy):
        want_plan = ref.plan(c.explicit, c.index_div, c.S, c.n_sym, n_cdfs, stride, fused_dq=c.fused, policy=c.policy)
        assert hip.rans_decode_path(c.explicit, c.index_div, c.S, c.n_sym, n_cdfs, stride, fused_dq=c.fused) == want_plan, name
        if not c.launch:
            return
        b = ref.build(c)
        d = _device(dev, c, b)
        # the device encoder on the same tables: the oracle's bytes, stream for stream
        ebuf, eoff, enb, est = hip.rans_encode_batch(d['sym'], d['cdfs'], d['sizes'], d['offs'], indexes=d['idx'], index_div=c.index_div,
                                                     out_stride=hip.rans_max_bytes(c.n_sym))
        assert int(est.max()) == 0 and _bytes_of(ebuf, eoff, enb) == b.streams, name
        want_sym = d['sym']
        if c.fused:
            assert hip.rans_decode_dequantize_supported(n_cdfs, stride)
            y1, st1, s1 = hip.rans_decode_dequantize_batch(d['buf'], d['off'], d['nb'], c.n_sym, d['cdfs'], d['sizes'], d['offs'], c.index_div,
                                                           d['med'], want_symbols=True)
            y0, st0, s0 = hip.rans_decode_dequantize_batch(d['buf'], d['off'], d['nb'], c.n_sym, d['cdfs'], d['sizes'], d['offs'], c.index_div,
                                                           d['med'], want_symbols=False)
            cs, cst, cy = _c_call(hip, dev, c, d)
            _, cst0, cy0 = _c_call(hip, dev, c, d, want_symbols=False)
            assert s0 is None and y1.shape == (c.S, c.HW, c.C) and y1.dtype == torch.bfloat16
            want_y = ref.dequantize_ref(b.sym, b.medians, c.HW).view(I16).to(dev)
            for y in (y1.view(I16), y0.view(I16), cy, cy0):
                assert torch.equal(y, want_y), name
            for st in (st1, st0, cst, cst0):
                assert int(st.abs().max()) == 0, name
            assert torch.equal(s1, want_sym) and torch.equal(cs, want_sym), name
            _, nhwc = hip.eb_dequantize(s1.reshape(c.S, c.C, c.HW, 1), d['med'], want_f32=False, want_nhwc=True)
            assert torch.equal(nhwc.reshape(c.S, c.HW, c.C).view(I16), y1.view(I16)), name
        else:
            s1, st1 = hip.rans_decode_batch(d['buf'], d['off'], d['nb'], c.n_sym, d['cdfs'], d['sizes'], d['offs'], indexes=d['idx'],
                                            index_div=c.index_div)
            cs, cst, _ = _c_call(hip, dev, c, d)
            assert int(st1.abs().max()) == 0 and int(cst.abs().max()) == 0, name
            assert torch.equal(s1, want_sym) and torch.equal(cs, want_sym), name


@pytest.mark.timeout(120)
@pytest.mark.parametrize('name', [c.name for c in ref.CASES if c.damage])
def test_new_paths_terminate_on_damaged_streams(S, dev, name):
    """The streams of test_rans_decoders_terminate_on_hostile_streams through the serial kernels this file newly reaches (lut8, ragged2
    at two waves, ragged 8-bit, generic-global) and the fused pass behind lut-u8: an all-0xFF stream, valid streams cut to 16 and to 8
    bytes.  Every loop of these kernels is bounded by the call's sizes -- they walk n_sym positions, an escape reads at most eight
    nibbles (decode_escape), the searches bisect a row, words past a stream's end are zeros -- so the launch returns; status bit 3 is
    set on exactly the damaged streams, every other stream (its y_hat rows included) is exact, the guards stay intact."""
    hip = S.hip
    c = ref.CASE_BY_NAME[name]
    b = ref.build(c)
    streams, which = ref.damage(b.streams)
    d = _device(dev, c, b, streams)
    with _policy(hip, c.policy):
        cs, cst, cy = _c_call(hip, dev, c, d)
    st = cst.cpu().numpy()
    good = np.array([i not in which for i in range(c.S)])
    assert ((st & 8) != 0).tolist() == (~good).tolist(), (name, st[which])
    assert not st[good].any(), name
    assert np.array_equal(cs.cpu().numpy()[good], b.sym[good]), name
    if c.fused:
        want_y = ref.dequantize_ref(b.sym, b.medians, c.HW).view(I16).numpy()
        assert np.array_equal(cy.cpu().numpy()[good], want_y[good]), name


def test_fused_call_refuses_what_it_does_not_take(S, dev):
    """sc2_rans_decode_dequantize_batch returns its documented code -- SC2_ERR_UNSUPPORTED (-2) for a channel count that is not a
    multiple of 8 or above 64, a row too long for the LUT decoders, n_sym != n_cdfs * index_div; SC2_ERR_INVALID_ARG (-1) for null
    medians / y_hat -- and touches none of its outputs."""
    hip = S.hip
    lib, p = hip.lib(), hip._ptr
    c = ref.CASE_BY_NAME['dq-reg C24 HW9 S65']
    b = ref.build(c)
    d = _device(dev, c, b)
    HW, n_streams = c.HW, c.S
    cdfs = torch.zeros((72, 4097), dtype=I32, device=dev)          # (large enough for every shape below; refused calls read none of it)
    sizes = torch.full((72,), 5, dtype=I32, device=dev)
    offs = torch.zeros((72,), dtype=I32, device=dev)
    med = torch.zeros((72,), dtype=torch.float32, device=dev)
    UNSUPPORTED, INVALID = -2, -1
    for what, C, stride, n_sym, has_med, has_y, want in (('12 channels', 12, 40, 12 * HW, True, True, UNSUPPORTED),
                                                         ('72 channels', 72, 40, 72 * HW, True, True, UNSUPPORTED),
                                                         ('cdf_stride 4097', 24, 4097, 24 * HW, True, True, UNSUPPORTED),
                                                         ('n_sym != C * index_div', 24, 40, 24 * HW - 1, True, True, UNSUPPORTED),
                                                         ('null medians', 24, 40, 24 * HW, False, True, INVALID),
                                                         ('null y_hat', 24, 40, 24 * HW, True, False, INVALID)):
        ws_bytes = int(lib.sc2_rans_workspace_bytes(n_streams, n_sym, C, stride))
        arenas = [_Arena(n_streams * 72 * HW, I32, dev), _Arena(n_streams * HW * 72, I16, dev), _Arena(n_streams, I32, dev),
                  _Arena(ws_bytes // 4, I32, dev)]
        a_sym, a_y, a_st, a_ws = arenas
        rc = lib.sc2_rans_decode_dequantize_batch(p(d['buf']), d['buf'].shape[1], p(d['off']), p(d['nb']), HW, n_streams, n_sym, p(cdfs), C, stride,
                                                  p(sizes), p(offs), p(med) if has_med else None, a_sym.ptr(), a_y.ptr() if has_y else None,
                                                  a_st.ptr(), a_ws.ptr(), ws_bytes, hip._stream())
        torch.cuda.synchronize()
        assert rc == want, (what, rc)
        assert lib.sc2_last_error(), what
        assert all(a.untouched() for a in arenas), what
    # the same arguments, as the call takes them, decode (the refusals above are not an artefact of the harness)
    _c_call(hip, dev, c, d)

