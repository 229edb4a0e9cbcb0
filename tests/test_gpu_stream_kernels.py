"""-m gpu: the grid-stride kernels that carry the training step's large tensors -- csrc/loss.hip (sc2_mse_sum_bf16, sc2_mse_grad_bf16,
sc2_relu_bwd_bf16, sc2_relu_bwd_mse_bf16), csrc/gdn_bwd.hip (sc2_gdn_bwd_pre, sc2_gdn_bwd_post, sc2_colsum_bf16) and the two layout
conversions of csrc/layout.hip -- against the float64 references of tests/ref_stream.py, element by element, PAST their grid caps.

The rest of the suite runs these kernels' first trip only (n8 <= 9 792, M = 198, 180 pixels) or inside end-to-end comparisons by
relative L2 norm (< 1.5e-2) and totals (1e-5): one lost 8-element chunk in 8 M elements is 1e-6 of such a total.  Here:

  dyadic operands   small integers (norm in {1, 2}, scale 0.5): every f32 intermediate is exact in any order of summation, with or
                    without FMA contraction, through the atomics too (tests/test_stream_ref_cpu.py proves the conditions on the
                    reference) -- every output has to EQUAL the float64 reference (as values: the sign of a zero is left open except
                    where a ReLU mask is shut, which is +0 bits).
  random operands   N(0, 1) as bf16, norm uniform in [0.5, 4].  bf16 outputs: every element |got - ref| <= 2^-8 |ref| + slack * scale,
                    scale = the sum of the magnitudes of the terms added; f32 sums: |got - ref| <= slack * sum |terms|; slack =
                    F32_MARGIN = 8 times the error of the float32 form of the SAME reference (ref_stream.E_F32_MAX, re-measured by
                    the CPU test) -- nothing measured on the kernel.  Pure selects and exact restatements are compared BIT FOR BIT
                    with the same f32 expression in torch: relu_bwd (with `add`: (g.float() + add.float()).to(bf16)), mse_grad
                    (s = 2.0f * scale), gdn_bwd_post, both layout conversions (torch's .to(bfloat16)).
  every launch      runs twice: once through the hip.* wrapper, once through the C entry point with every output inside a
                    sentinel-filled arena of exactly its declared extent (partial: sc2_mse_partial_len floats, d_beta / colsum: C
                    floats) -- guards intact, every element written, and the two results bit-equal (d_beta / colsum on random
                    operands excepted: f32 atomics).  The arena also keeps a kernel that skips a trip from being handed the right
                    answer in recycled memory.
  grids             what the library reports (sc2_mse_partial_len, sc2_gdn_bwd_pre_blocks, sc2_colsum_blocks,
                    sc2_gdn_bwd_post_blocks, sc2_layout_blocks) equals ref_stream.launch() for every case.

Cases (the smallest shapes that reach each path; ref_stream.*_CASES):

  loss.hip, all four kernels; grid clamp(ceil(n8 / 256), 1, 4096), n8 = n / 8
      n8         reaches
      1          one live lane, partial_len 1
      257        a second workgroup with one lane
      1 048 576  the cap exactly, one trip
      1 048 577  exactly one thread takes a second trip
      2 097 452  a ragged third trip (300 chunks)

  gdn_bwd_pre, both directions; cpr = C / 8, ppi = 256 // cpr, nb = min(ceil(M / ppi), 1024), pixels m and m + nb ppi per iteration
      C, M          reaches
      8, 1          cpr 1, 255 threads without a pixel
      40, 198       ppi 51, one idle thread, nb 4
      48, 43 009    nb capped, exactly one thread with `two`
      48, 86 059    every thread `two`, then a ragged second iteration without it
      1032, 100     cpr 129, 127 idle
      2040, 37      cpr 255
      2048, 3 073   ppi 1, capped, second iteration with and without `two`

  colsum; 1 024 threads, ppi = 1024 // cpr, nb = min(ceil(M / ppi), 256), four pixels per iteration
      8, 1          smallest case
      40, 1 000     ppi 204, 4 idle
      96, 198       unroll slots 1..3 never live
      96, 21 761    nb capped, one thread with slot 1 live
      96, 87 140    a ragged second iteration
      2040, 37      cpr 255
      2048, 4 101   ppi 4, second iteration with slot 0 only

  gdn_bwd_post; grid min(ceil(n8 / 256), 8192): n8 = 1, 257, 2 097 153 (one thread in a second trip); x carries +0, -0 and both signs
  at fixed positions of the first and the last chunk.

  layout; grid min(ceil(pixels / 256), 16384) x channel groups
      N, C, H, W, Cpad          reaches
      3, 5, 6, 10, 8            the small case of test_layout_roundtrip
      2, 9, 3, 7, 12            the 4-wide kernel, with a group of one live channel
      2, 3, 5, 5, 16            whole groups of padding
      5, 3, 1, 838 861, 4       4 194 305 pixels: one pixel past the cap, on the 4-wide kernel; the thread's image index changes
      5, 8, 1, 838 861, 8       the same on the 8-wide kernel
  and back (sc2_nhwc_bf16_to_nchw_f32): (3, 24, 6, 10), (5, 8, 1, 838 861).  The forward's input carries +-0, +-inf, NaN, f32
  subnormals, the largest finite f32 and the neighbourhood of bf16 ties at fixed positions, the last pixel among them: torch's
  .to(bfloat16) bit for bit (a NaN: only "is NaN").

Also: ReLU masks on +0, -0 and the smallest bf16 subnormals of both signs (the mask is out > 0: a positive subnormal passes the
gradient) with +-inf and NaN in g (through where the mask is open, exactly +0 where it is shut); the refusals the launchers state
(n % 8, C % 8, C / 8 > 256, Cpad < C, null pointers: the documented code, nothing written).
Measured on an MI355X (profiles/r26_gpu_stream_tests.log), largest over all cases, next to the bound: mse_sum partials
1.6e-7 (1.48e-6), d_beta 3.1e-7 (1.44e-6), colsum 1.7e-8 (1.33e-7); d_norm, dx_direct and relu_bwd_mse 0 beyond the one bf16 rounding
(2.2e-6, 9.1e-7, 9.0e-7).  No test failed on the kernels as they were.
"""
import ctypes

import pytest
import torch

import ref_stream as R

pytestmark = pytest.mark.gpu

BOUND = {k: R.F32_MARGIN * v for k, v in R.E_F32_MAX.items()}
BF, F32 = torch.bfloat16, torch.float32
_cases = {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a).view(-1), _bits(b).view(-1))


def _same_values(got, want64):
    """got (bf16 / f32) equals the float64 reference as values, nothing non-finite."""
    g = got.double().reshape(-1)
    return bool(torch.isfinite(g).all()) and torch.equal(g, want64.reshape(-1))


def _report(tag, errors, failures):
    print(tag + ': ' + '  '.join('{} {:.2e} ({:.2e})'.format(k, e, BOUND[k.split('/')[0]]) for k, e in errors.items()))
    failures.extend((tag, k, e, BOUND[k.split('/')[0]]) for k, e in errors.items() if not e <= BOUND[k.split('/')[0]])


class _Arena(object):
    """`n` elements of bf16 (as int16) or f32 (as int32) between two bands of PAD sentinel elements."""
    PAD = 4096                              # (elements: the payload stays 16-byte aligned)

    def __init__(self, n, dtype, dev):
        self.int_dtype, self.sentinel = (torch.int16, 0x5A5A) if dtype == BF else (torch.int32, 0x5A5A5A5A)
        self.n, self.dtype = n, dtype
        self.buf = torch.full((n + 2 * self.PAD,), self.sentinel, dtype=self.int_dtype, device=dev)
        assert self.buf.data_ptr() % 16 == 0

    def payload(self):
        return self.buf[self.PAD:self.PAD + self.n].view(self.dtype)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.PAD * self.buf.element_size())

    def intact(self):
        """guards untouched, every payload element written"""
        return (bool((self.buf[:self.PAD] == self.sentinel).all()) and bool((self.buf[self.PAD + self.n:] == self.sentinel).all()),
                not bool((self.buf[self.PAD:self.PAD + self.n] == self.sentinel).any()))


def _in_arenas(dev, spec, call, what):
    """spec: [(elements, dtype)]; call(ptr, ...) launches through the C entry point -> the payloads, after the checks."""
    arenas = [_Arena(n, dt, dev) for n, dt in spec]
    assert call(*[a.ptr() for a in arenas]) == 0, what
    torch.cuda.synchronize()
    for i, a in enumerate(arenas):
        guards, written = a.intact()
        assert guards, '{}: a write outside output {}'.format(what, i)
        assert written, '{}: an element of output {} was left unwritten'.format(what, i)
    return [a.payload() for a in arenas]


def _on_device(c, dev):
    """the operands as bf16 on the device (rounded on the host, where they are bf16 values already: tests/test_stream_ref_cpu.py)"""
    return {k: (v.to(BF).to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _case(maker, dev, *a):
    key = (maker.__name__,) + a
    if key in _cases:
        return _cases[key]
    d = _on_device(maker(*a), dev)
    if sum(v.numel() for v in d.values() if isinstance(v, torch.Tensor)) <= 1 << 22:      # (the large cases run once: not kept)
        _cases[key] = d
    return d


def test_reported_grids_are_the_restated_launch_arithmetic(S, dev):
    lib = S.hip.lib()
    for n8 in R.LOSS_N8 + (256, 1048575, 4096 * 256 * 2, 4096 * 256 * 2 + 1):
        assert lib.sc2_mse_partial_len(8 * n8) == R.launch('loss', 8 * n8)['blocks'], n8
    assert lib.sc2_mse_partial_len(0) == 0 and lib.sc2_mse_partial_len(-8) == 0
    for C, M in R.PRE_CASES + ((48, 43008), (48, 86016), (2048, 1024), (2048, 1025), (8, 10 ** 9)):
        assert lib.sc2_gdn_bwd_pre_blocks(M, C) == R.launch('gdn_bwd_pre', M, C)['blocks'], (C, M)
    for C, M in R.COLSUM_CASES + ((96, 21760), (96, 87040), (2048, 1024), (2048, 1025), (8, 10 ** 9)):
        assert lib.sc2_colsum_blocks(M, C) == R.launch('colsum', M, C)['blocks'], (C, M)
    for f in (lib.sc2_gdn_bwd_pre_blocks, lib.sc2_colsum_blocks):
        assert f(5, 12) == 0 and f(5, 2056) == 0 and f(0, 8) == 0 and f(5, 0) == 0 and f(-1, 8) == 0
    for n8 in R.POST_N8 + (256, 2097152, 8192 * 256 * 3):
        assert lib.sc2_gdn_bwd_post_blocks(8 * n8) == R.launch('gdn_bwd_post', 8 * n8)['blocks'], n8
    assert lib.sc2_gdn_bwd_post_blocks(12) == 0 and lib.sc2_gdn_bwd_post_blocks(0) == 0 and lib.sc2_gdn_bwd_post_blocks(-8) == 0
    for pixels in [N * H * W for N, C, H, W, _ in R.LAYOUT_CASES] + [1, 256, 257, 4194304, 4194305, 10 ** 10]:
        assert lib.sc2_layout_blocks(pixels) == R.launch('layout', pixels)['blocks'], pixels
    assert lib.sc2_layout_blocks(0) == 0 and lib.sc2_layout_blocks(-5) == 0


# ---- csrc/loss.hip ----

def _loss_launches(S, dev, c):
    """Every kernel of loss.hip on the operands of c, each through the wrapper and through the C entry point into arenas -> dict."""
    hip, lib = S.hip, S.hip.lib()
    n, st = c['n'], hip._stream()
    scale = torch.tensor([c['scale']], dtype=F32, device=dev)
    p = hip._ptr
    out = {}
    plen = int(lib.sc2_mse_partial_len(n))
    parts = [_in_arenas(dev, [(plen, F32)], lambda o: lib.sc2_mse_sum_bf16(p(c['x']), p(c['y']), n, o, st), 'mse_sum')[0] for _ in range(2)]
    assert _same_bits(*parts), 'two mse_sum launches differ'
    assert _same_bits(hip.mse_sum(c['x'], c['y']).view(1), parts[0].double().sum().float().view(1))
    out['partial'] = parts[0]

    def both(name, wrapper, c_call):
        a = wrapper()
        assert a.dtype == BF and a.shape == (n,)
        b = _in_arenas(dev, [(n, BF)], c_call, name)[0]
        assert _same_bits(a, b), 'two {} launches differ'.format(name)
        out[name] = a
    both('mse_grad', lambda: hip.mse_grad(c['x'], c['y'], scale), lambda o: lib.sc2_mse_grad_bf16(p(c['x']), p(c['y']), n, p(scale), o, st))
    both('relu_bwd', lambda: hip.relu_bwd(c['g'], c['out']), lambda o: lib.sc2_relu_bwd_bf16(p(c['g']), p(c['out']), None, n, o, st))
    both('relu_bwd_add', lambda: hip.relu_bwd(c['g'], c['out'], c['add']),
         lambda o: lib.sc2_relu_bwd_bf16(p(c['g']), p(c['out']), p(c['add']), n, o, st))
    for has_g, relu in R.MSE_VARIANTS:
        g = c['g'] if has_g else None
        both('relu_bwd_mse/g{:d}relu{:d}'.format(has_g, relu), lambda: hip.relu_bwd_mse(g, c['out'], c['t'], scale, relu=relu),
             lambda o: lib.sc2_relu_bwd_mse_bf16(p(g), p(c['out']), p(c['t']), p(scale), n, int(relu), o, st))
    return out, scale


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('n8', R.LOSS_N8)
def test_loss_kernels_element_by_element(S, dev, n8, kind):
    c = _case(R.make_loss_case, dev, n8, kind)
    L = R.launch('loss', c['n'])
    assert S.hip.lib().sc2_mse_partial_len(c['n']) == L['blocks']
    got, scale = _loss_launches(S, dev, c)
    assert got['partial'].shape == (L['blocks'],)
    zero = torch.zeros((), dtype=BF, device=dev)
    shut = c['out'] <= 0
    failures, errors = [], {}
    ref_partial = R.mse_sum(c['x'], c['y'], L['blocks'])
    # selects and exact restatements: the same f32 expression in torch, bit for bit, on either kind of operands
    s = torch.full((), 2.0, dtype=F32, device=dev) * scale[0]
    assert _same_bits(got['mse_grad'], (s * (c['x'].float() - c['y'].float())).to(BF)), 'mse_grad'
    assert _same_bits(got['relu_bwd'], torch.where(c['out'] > 0, c['g'], zero)), 'relu_bwd'
    assert _same_bits(got['relu_bwd_add'], torch.where(c['out'] > 0, (c['g'].float() + c['add'].float()).to(BF), zero)), 'relu_bwd + add'
    if kind == 'dyadic':
        assert _same_values(got['partial'], ref_partial), 'mse_sum partials'
        assert _same_values(got['mse_grad'], R.mse_grad(c['x'], c['y'], c['scale'])), 'mse_grad'
        assert _same_values(got['relu_bwd'], R.relu_bwd(c['g'], c['out'])) and _same_values(got['relu_bwd_add'], R.relu_bwd(c['g'], c['out'], c['add']))
    else:
        errors['mse_sum'] = R.err(got['partial'], ref_partial, ref_partial)
    for has_g, relu in R.MSE_VARIANTS:
        name = 'relu_bwd_mse/g{:d}relu{:d}'.format(has_g, relu)
        ref, sc = R.relu_bwd_mse(c['g'] if has_g else None, c['out'], c['t'], c['scale'], relu)
        if kind == 'dyadic':
            assert _same_values(got[name], ref), name
        else:
            errors[name] = R.err_bf16(got[name], ref, sc)
        if relu:
            assert bool((_bits(got[name])[shut] == 0).all()), name + ': not +0 where the mask is shut'
    for name in ('relu_bwd', 'relu_bwd_add'):
        assert bool((_bits(got[name])[shut] == 0).all()), name + ': not +0 where the mask is shut'
    _report('loss n8 {} {}'.format(n8, kind), errors, failures)
    assert not failures, failures


def test_relu_masks_on_zeros_and_subnormals_with_inf_and_nan_gradients(S, dev):
    """out: +0, -0, +-2^-133 (the smallest bf16 subnormals), +-1 against g: +inf, -inf, NaN, in every combination from element 16 on and
    eight of them in the last chunk.  The mask is out > 0: open for 2^-133 and 1 only.  The reference is computed on the host."""
    n8 = 257
    c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in R.make_loss_case(n8, 'random').items()}
    n = c['n']
    inf, nan = float('inf'), float('nan')
    combos = [(o, g) for o in (0.0, -0.0, R.SUB, -R.SUB, 1.0, -1.0) for g in (inf, -inf, nan)]
    where = list(range(16, 16 + len(combos))) + list(range(n - 8, n))
    vals = combos + [(R.SUB, inf), (R.SUB, nan), (-R.SUB, inf), (-0.0, nan), (0.0, -inf), (1.0, nan), (-1.0, inf), (R.SUB, -inf)]
    for i, (o, g) in zip(where, vals):
        c['out'][i], c['g'][i] = o, g
    assert torch.equal(R.bf16(c['out']), c['out']) and int((c['out'] == R.SUB).sum()) == 6
    d = _on_device(c, dev)
    assert _same_bits(d['out'].cpu(), c['out'].to(BF))
    got, _ = _loss_launches(S, dev, d)
    got = {k: v.cpu() for k, v in got.items()}
    idx = torch.tensor(where)
    rest = torch.ones(n, dtype=torch.bool)
    rest[idx] = False
    is_open = c['out'] > 0
    assert is_open[idx].tolist() == [o > 0 for o, _ in vals] and sum(o == R.SUB for o, _ in vals) == 6
    zero = torch.zeros((), dtype=BF)
    assert _same_bits(got['relu_bwd'], torch.where(is_open, c['g'].to(BF), zero))                    # a select: NaN payload and all
    failures, errors = [], {}

    def special(name, ref):
        g = got[name].double()[idx]
        r = ref[idx]
        assert torch.equal(torch.isnan(g), torch.isnan(r)), name + ': NaN where none belongs, or none where one does'
        assert torch.equal(g[~torch.isnan(r)], r[~torch.isnan(r)]), name + ': an inf did not come through, or came through a shut mask'
    ref = R.relu_bwd(c['g'], c['out'], c['add'])
    special('relu_bwd_add', ref)
    assert torch.equal(got['relu_bwd_add'][rest], ref.float().to(BF)[rest])
    for has_g, relu in R.MSE_VARIANTS:
        name = 'relu_bwd_mse/g{:d}relu{:d}'.format(has_g, relu)
        ref, sc = R.relu_bwd_mse(c['g'] if has_g else None, c['out'], c['t'], c['scale'], relu)
        if has_g:
            special(name, ref)
            errors[name] = R.err_bf16(got[name][rest], ref[rest], sc[rest])
        else:
            errors[name] = R.err_bf16(got[name], ref, sc)                  # (no g: every element is finite, the subnormals too)
        if relu:
            assert bool((_bits(got[name])[~is_open] == 0).all()), name + ': not +0 where the mask is shut'
            assert bool((got[name][c['out'] == R.SUB] != 0).all()), name + ': a positive subnormal did not pass the gradient'
    for name in ('relu_bwd', 'relu_bwd_add'):
        assert bool((_bits(got[name])[~is_open] == 0).all()) and bool((got[name][c['out'] == R.SUB] != 0).all()), name
    _report('relu special values', errors, failures)
    assert not failures, failures


# ---- csrc/gdn_bwd.hip ----

@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C,M', R.PRE_CASES)
def test_gdn_bwd_pre_element_by_element(S, dev, C, M, kind):
    hip, lib = S.hip, S.hip.lib()
    c = _case(R.make_pre_case, dev, C, M, kind)
    assert lib.sc2_gdn_bwd_pre_blocks(M, C) == R.launch('gdn_bwd_pre', M, C)['blocks']
    p, st = hip._ptr, hip._stream()
    failures = []
    for inverse in (False, True):
        ref = R.gdn_bwd_pre(c['gy'], c['x'], c['norm'], inverse)
        d_norm, dxd, d_beta = hip.gdn_bwd_pre(c['gy'], c['x'], c['norm'], inverse)
        assert d_norm.shape == dxd.shape == (M, C) and d_norm.dtype == dxd.dtype == BF and d_beta.shape == (C,) and d_beta.dtype == F32
        a_norm, a_dxd, a_beta = _in_arenas(
            dev, [(M * C, BF), (M * C, BF), (C, F32)],
            lambda o1, o2, o3: lib.sc2_gdn_bwd_pre(p(c['gy']), p(c['x']), p(c['norm']), M, C, int(inverse), o1, o2, o3, st), 'gdn_bwd_pre')
        assert _same_bits(d_norm, a_norm) and _same_bits(dxd, a_dxd), 'two gdn_bwd_pre launches differ'
        tag = 'gdn_bwd_pre {}x{} {} inverse {:d}'.format(C, M, kind, inverse)
        if kind == 'dyadic':
            assert _same_bits(d_beta, a_beta), 'd_beta of two launches differs on exact operands'
            assert _same_values(d_norm, ref['d_norm']), tag + ' d_norm'
            assert _same_values(dxd, ref['dx_direct']), tag + ' dx_direct'
            assert _same_values(d_beta, ref['d_beta']), tag + ' d_beta'
        else:
            errors = {'d_norm': R.err_bf16(d_norm, ref['d_norm'], ref['d_norm'].abs()),
                      'dx_direct': R.err_bf16(dxd, ref['dx_direct'], ref['dx_direct'].abs()),
                      'd_beta': max(R.err(d_beta, ref['d_beta'], ref['d_beta_scale']), R.err(a_beta, ref['d_beta'], ref['d_beta_scale']))}
            _report(tag, errors, failures)
    assert not failures, failures


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C,M', R.COLSUM_CASES)
def test_colsum_element_by_element(S, dev, C, M, kind):
    hip, lib = S.hip, S.hip.lib()
    c = _case(R.make_colsum_case, dev, C, M, kind)
    assert lib.sc2_colsum_blocks(M, C) == R.launch('colsum', M, C)['blocks']
    ref, sc = R.colsum(c['x'])
    got = hip.colsum_bf16(c['x'], C)
    again = _in_arenas(dev, [(C, F32)], lambda o: lib.sc2_colsum_bf16(hip._ptr(c['x']), M, C, o, hip._stream()), 'colsum')[0]
    assert got.shape == (C,) and got.dtype == F32
    failures = []
    if kind == 'dyadic':
        assert _same_bits(got, again) and _same_values(got, ref)
    else:
        _report('colsum {}x{}'.format(C, M), {'colsum': max(R.err(got, ref, sc), R.err(again, ref, sc))}, failures)
    assert not failures, failures


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('n8', R.POST_N8)
def test_gdn_bwd_post_element_by_element(S, dev, n8, kind):
    hip, lib = S.hip, S.hip.lib()
    c = _case(R.make_post_case, dev, n8, kind)
    n = c['n']
    assert lib.sc2_gdn_bwd_post_blocks(n) == R.launch('gdn_bwd_post', n)['blocks']
    got = hip.gdn_bwd_post(c['dx_direct'], c['x'], c['t'])
    again = _in_arenas(dev, [(n, BF)], lambda o: lib.sc2_gdn_bwd_post(hip._ptr(c['dx_direct']), hip._ptr(c['x']), hip._ptr(c['t']), n, o,
                                                                       hip._stream()), 'gdn_bwd_post')[0]
    assert _same_bits(got, again), 'two gdn_bwd_post launches differ'
    want = (c['dx_direct'].float() + R.sign(c['x'].float()) * c['t'].float()).to(BF)                  # one f32 addition, one rounding
    assert _same_bits(got, want)
    for base in (0, n - 8):                                            # +-0 in x: the direct term alone
        assert _same_bits(got[base:base + 2], c['dx_direct'][base:base + 2]) and not _same_bits(got[base + 2:base + 4], c['dx_direct'][base + 2:base + 4])
    if kind == 'dyadic':
        assert _same_values(got, R.gdn_bwd_post(c['dx_direct'], c['x'], c['t']))


# ---- csrc/layout.hip ----

@pytest.mark.parametrize('N,C,H,W,cpad', R.LAYOUT_CASES)
def test_nchw_f32_to_nhwc_bf16_bit_for_bit(S, dev, N, C, H, W, cpad):
    hip, lib = S.hip, S.hip.lib()
    x_host, pos = R.make_layout_case(N, C, H, W)
    x = x_host.to(dev)
    assert lib.sc2_layout_blocks(N * H * W) == R.launch('layout', N * H * W)['blocks']
    got = hip.nchw_f32_to_nhwc_bf16(x, cpad)
    again = _in_arenas(dev, [(N * H * W * cpad, BF)], lambda o: lib.sc2_nchw_f32_to_nhwc_bf16(hip._ptr(x), o, N, C, H, W, cpad, hip._stream()),
                       'nchw_to_nhwc')[0]
    assert got.shape == (N, H, W, cpad) and got.dtype == BF
    g, a = _bits(got).view(N, H * W, cpad).clone(), _bits(again).view(N, H * W, cpad).clone()
    want = _bits(R.nchw_to_nhwc_bf16(x, cpad)).view(N, H * W, cpad).clone()
    sp = R.layout_specials()
    host = _bits(sp.to(BF))                                             # the specials' expected bits: the host's conversion
    assert (N - 1, C - 1, H * W - 1) in pos
    for k, (n, ch, px) in enumerate(pos):
        k = k % len(sp)
        if bool(torch.isnan(sp[k])):
            for t in (got, again):
                assert bool(torch.isnan(t.view(N, H * W, cpad)[n, px, ch])), 'a NaN became a number'
            g[n, px, ch] = a[n, px, ch] = want[n, px, ch] = 0
        else:
            want[n, px, ch] = host[k]
    assert torch.equal(g, a), 'two launches differ'
    assert bool((g[..., C:] == 0).all()), 'padding channels are not +0'
    bad = (g != want).nonzero()
    assert bad.numel() == 0, 'first differing (image, pixel, channel): {} of {}'.format(bad[0].tolist(), bad.shape[0])


@pytest.mark.parametrize('N,C,H,W', R.LAYOUT_BACK_CASES)
def test_nhwc_bf16_to_nchw_f32_bit_for_bit(S, dev, N, C, H, W):
    hip, lib = S.hip, S.hip.lib()
    gen = torch.Generator().manual_seed(N * C + W)
    x = torch.randn(N, H, W, C, generator=gen).to(dev).to(BF)
    flat = x.view(-1)
    for k, v in enumerate((0.0, -0.0, float('inf'), float('-inf'), R.SUB, -R.SUB)):
        flat[k * 3], flat[flat.numel() - 1 - k * 5] = v, v
    assert lib.sc2_layout_blocks(N * H * W) == R.launch('layout', N * H * W)['blocks']
    got = hip.nhwc_bf16_to_nchw_f32(x)
    again = _in_arenas(dev, [(N * C * H * W, F32)], lambda o: lib.sc2_nhwc_bf16_to_nchw_f32(hip._ptr(x), o, N, C, H, W, hip._stream()),
                       'nhwc_to_nchw')[0]
    assert got.shape == (N, C, H, W) and got.dtype == F32 and _same_bits(got, again)
    assert _same_bits(got, R.nhwc_bf16_to_nchw(x))                       # (a bf16 IS the upper half of its f32: torch's cast is exact)


# ---- the arenas by name, the refusals ----

@pytest.mark.parametrize('n8', [257, 1048577], ids=['small', 'capped'])
def test_loss_outputs_stay_inside_their_extents(S, dev, n8):
    """Every output of loss.hip inside a sentinel-filled arena of exactly its extent (partial: sc2_mse_partial_len(n) floats): guards
    intact, every element written (_loss_launches asserts both for each kernel)."""
    c = _case(R.make_loss_case, dev, n8, 'dyadic')
    got, _ = _loss_launches(S, dev, c)
    assert got['partial'].numel() == S.hip.lib().sc2_mse_partial_len(c['n']) == R.launch('loss', c['n'])['blocks'] and len(got) == 8


@pytest.mark.parametrize('C,M', [(40, 198), (48, 43009)], ids=['small', 'capped'])
def test_gdn_bwd_outputs_stay_inside_their_extents(S, dev, C, M):
    """d_norm, dx_direct (M C bf16), d_beta (exactly C floats), dx and the column sums (C floats) inside arenas, through the C entry points."""
    hip, lib = S.hip, S.hip.lib()
    c = _case(R.make_pre_case, dev, C, M, 'dyadic')
    p, st = hip._ptr, hip._stream()
    d_norm, dxd, d_beta = _in_arenas(dev, [(M * C, BF), (M * C, BF), (C, F32)],
                                     lambda o1, o2, o3: lib.sc2_gdn_bwd_pre(p(c['gy']), p(c['x']), p(c['norm']), M, C, 0, o1, o2, o3, st), 'gdn_bwd_pre')
    t = d_norm.clone()
    dx, = _in_arenas(dev, [(M * C, BF)], lambda o: lib.sc2_gdn_bwd_post(p(dxd), p(c['x']), p(t), M * C, o, st), 'gdn_bwd_post')
    cs, = _in_arenas(dev, [(C, F32)], lambda o: lib.sc2_colsum_bf16(p(t), M, C, o, st), 'colsum')
    ref = R.gdn_bwd_pre(c['gy'], c['x'], c['norm'], False)
    assert _same_values(d_beta, ref['d_beta']) and _same_values(cs, ref['d_beta'])         # (dyadic: d_norm is exact in bf16 too)
    assert _same_values(dx, R.gdn_bwd_post(ref['dx_direct'], c['x'], ref['d_norm']))


def test_refusals(S, dev):
    """What the launchers refuse: the documented code (SC2_ERR_INVALID_ARG), nothing written -- d_beta / colsum not zeroed either."""
    hip, lib = S.hip, S.hip.lib()
    p, st = hip._ptr, hip._stream()
    b = torch.ones(4096, dtype=BF, device=dev)
    f = torch.ones(4096, dtype=F32, device=dev)
    o1, o2 = torch.full((4096,), 3.0, dtype=BF, device=dev), torch.full((4096,), 3.0, dtype=BF, device=dev)
    of = torch.full((4096,), 3.0, dtype=F32, device=dev)
    rcs = []
    for n in (12, 0, -8):
        rcs += [lib.sc2_mse_sum_bf16(p(b), p(b), n, p(of), st), lib.sc2_mse_grad_bf16(p(b), p(b), n, p(f), p(o1), st),
                lib.sc2_relu_bwd_bf16(p(b), p(b), None, n, p(o1), st), lib.sc2_relu_bwd_mse_bf16(p(b), p(b), p(b), p(f), n, 1, p(o1), st),
                lib.sc2_gdn_bwd_post(p(b), p(b), p(b), n, p(o1), st)]
    for M, C in ((4, 12), (1, 2056), (0, 8), (4, 0)):
        rcs += [lib.sc2_gdn_bwd_pre(p(b), p(b), p(b), M, C, 0, p(o1), p(o2), p(of), st), lib.sc2_colsum_bf16(p(b), M, C, p(of), st)]
    rcs += [lib.sc2_nchw_f32_to_nhwc_bf16(p(f), p(o1), 1, 5, 2, 2, 4, st), lib.sc2_nchw_f32_to_nhwc_bf16(p(f), p(o1), 1, 3, 2, 2, 6, st),
            lib.sc2_nchw_f32_to_nhwc_bf16(p(f), p(o1), 0, 3, 2, 2, 4, st), lib.sc2_nhwc_bf16_to_nchw_f32(p(b), p(of), 1, 12, 2, 2, st)]
    # null pointers, one at a time
    rcs += [lib.sc2_mse_sum_bf16(None, p(b), 64, p(of), st), lib.sc2_mse_sum_bf16(p(b), p(b), 64, None, st),
            lib.sc2_mse_grad_bf16(p(b), p(b), 64, None, p(o1), st), lib.sc2_mse_grad_bf16(p(b), p(b), 64, p(f), None, st),
            lib.sc2_relu_bwd_bf16(None, p(b), None, 64, p(o1), st), lib.sc2_relu_bwd_bf16(p(b), None, None, 64, p(o1), st),
            lib.sc2_relu_bwd_mse_bf16(None, None, p(b), p(f), 64, 1, p(o1), st), lib.sc2_relu_bwd_mse_bf16(None, p(b), None, p(f), 64, 1, p(o1), st),
            lib.sc2_relu_bwd_mse_bf16(None, p(b), p(b), None, 64, 0, p(o1), st),
            lib.sc2_gdn_bwd_pre(p(b), None, p(b), 4, 8, 0, p(o1), p(o2), p(of), st), lib.sc2_gdn_bwd_pre(p(b), p(b), p(b), 4, 8, 0, p(o1), p(o2), None, st),
            lib.sc2_gdn_bwd_post(p(b), p(b), None, 64, p(o1), st), lib.sc2_colsum_bf16(None, 4, 8, p(of), st), lib.sc2_colsum_bf16(p(b), 4, 8, None, st),
            lib.sc2_nchw_f32_to_nhwc_bf16(None, p(o1), 1, 3, 2, 2, 4, st), lib.sc2_nhwc_bf16_to_nchw_f32(p(b), None, 1, 8, 2, 2, st)]
    torch.cuda.synchronize()
    assert rcs == [-1] * len(rcs), rcs
    assert bool((o1 == 3.0).all()) and bool((o2 == 3.0).all()) and bool((of == 3.0).all())
    with pytest.raises(ValueError):
        hip.gdn_bwd_post(b[:12], b[:12], b[:12])
    with pytest.raises(ValueError):
        hip.gdn_bwd_pre(b[:24].view(2, 12), b[:24].view(2, 12), b[:24].view(2, 12), False)
    with pytest.raises(ValueError):
        hip.colsum_bf16(b[:24].view(2, 12), 12)
    with pytest.raises(ValueError):
        hip.nchw_f32_to_nhwc_bf16(f[:20].view(1, 5, 2, 2), 4)
