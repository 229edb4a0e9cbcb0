"""CPU: tests/ref_stream.py -- the float64 references tests/test_gpu_stream_kernels.py holds the streaming kernels of csrc/loss.hip,
csrc/gdn_bwd.hip and csrc/layout.hip against -- is itself proved against torch autograd, its case tables are tied to the restated
launch arithmetic, the dyadic operands are proved exact, and its float32 form is calibrated.

* reference against torch: gdn_bwd_pre, an exact float64 gamma^T product and gdn_bwd_post equal autograd of x / (beta + gamma |x|) and
  of x (beta + gamma |x|) within 1e-12 (dx and d_beta); relu_bwd_mse equals autograd of relu (or the identity) followed by
  <g, .> + scale sum((. - t)^2), at the relu's input where the kernel's mask (out > 0) and autograd's agree; mse_grad is the same
  without g; the mse_sum partials add up to the plain sum.
* launch(): every case reaches the trip it is listed for (second workgroup with one lane, the cap exactly, one thread in a second trip,
  a ragged third; exactly one thread with `two`, every thread with `two` then a ragged iteration without; unroll slots never / once
  live; ...).
* dyadic operands: for every case, (the sum of the magnitudes of the terms of every f32 sum) / unit < 2^24 -- so the sum is exact in
  f32 in ANY order, through the atomics too -- and every element-wise output is a bf16 value.  The condition is on the reference, never
  on the kernel.  The chunk or pixel that only the last ragged trip reaches contributes a nonzero amount to its sum.
* calibration: the float32 form against the float64 form on the random operands, under the metrics of ref_bn.py:

      loss n8    mse_sum   relu_bwd_mse     gdn_bwd_pre C, M  d_norm    dx_direct d_beta       colsum C, M   colsum
      1          4.34e-08  4.48e-08         8     1           1.79e-07  7.95e-08  1.79e-07     8     1       0.00e+00
      257        6.40e-08  8.32e-08         40    198         2.28e-07  1.14e-07  3.25e-08     40    1000    6.19e-09
      1048576    1.53e-07  9.01e-08         48    43009       2.72e-07  1.14e-07  5.20e-09     96    198     6.47e-09
      1048577    1.56e-07  9.03e-08         48    86059       2.72e-07  1.14e-07  3.33e-09     96    21761   1.93e-09
      2097452    1.85e-07  1.12e-07         1032  100         2.44e-07  1.14e-07  9.66e-08     96    87140   1.14e-09
                                            2040  37          2.59e-07  1.14e-07  1.50e-07     2040  37      1.65e-08
                                            2048  3073        2.72e-07  1.14e-07  2.41e-08     2048  4101    5.79e-09

  The maxima, rounded up in the third digit, are ref_stream.E_F32_MAX.  All are a few units of 2^-24 = 6e-8 of the condition scale: a
  thread's 8 to 24 squares added one after the other for mse_sum, the three roundings of -(g r) x r for d_norm, two for g r and for
  g + s (out - t); d_beta is largest where a column has one term (its own three roundings) and small where many terms of both signs
  cancel, as the column sums are.  The test re-measures every row, fails if a figure exceeds its constant and if a maximum falls below
  0.9 x its constant (a constant that has come loose from what it measures).
"""
import pytest
import torch

import ref_stream as R

_cache = {}
_measured = {}


def _case(maker, *a):
    key = (maker.__name__,) + a
    if key not in _cache:
        c = maker(*a)
        if sum(v.numel() for v in c.values() if isinstance(v, torch.Tensor)) > 1 << 24:
            return c                                                  # (the largest cases are not kept)
        _cache[key] = c
    return _cache[key]


def test_cases_reach_what_they_are_listed_for():
    L = {n8: R.launch('loss', 8 * n8) for n8 in R.LOSS_N8}
    assert (L[1]['blocks'], L[1]['trips'], L[1]['last_trip']) == (1, 1, 1)
    assert (L[257]['blocks'], L[257]['trips']) == (2, 1) and 257 - 256 == 1
    assert (L[1048576]['blocks'], L[1048576]['uncapped'], L[1048576]['trips'], L[1048576]['last_trip']) == (4096, 4096, 1, 1048576)
    assert (L[1048577]['blocks'], L[1048577]['uncapped'], L[1048577]['trips'], L[1048577]['last_trip']) == (4096, 4097, 2, 1)
    assert (L[2097452]['blocks'], L[2097452]['trips'], L[2097452]['last_trip']) == (4096, 3, 300)
    P = {c: R.launch('gdn_bwd_pre', c[1], c[0]) for c in R.PRE_CASES}
    assert (P[8, 1]['cpr'], P[8, 1]['ppi'], P[8, 1]['idle'], P[8, 1]['blocks'], P[8, 1]['last_live']) == (1, 256, 0, 1, (1, 0))
    assert (P[40, 198]['ppi'], P[40, 198]['idle'], P[40, 198]['blocks'], P[40, 198]['iters'], P[40, 198]['last_live']) == (51, 1, 4, 1, (198, 0))
    p = P[48, 43009]
    assert (p['cpr'], p['ppi'], p['idle'], p['blocks'], p['uncapped'], p['iters'], p['last_live']) == (6, 42, 4, 1024, 1025, 1, (43008, 1))
    assert R.launch('gdn_bwd_pre', 43008, 48)['uncapped'] == 1024 and R.launch('gdn_bwd_pre', 43008, 48)['last_live'] == (43008, 0)
    p = P[48, 86059]
    assert (p['blocks'], p['iters'], p['last_live']) == (1024, 2, (43, 0)) and 86059 - 43 == 2 * p['stride']
    assert (P[1032, 100]['cpr'], P[1032, 100]['ppi'], P[1032, 100]['idle'], P[1032, 100]['blocks']) == (129, 1, 127, 100)
    assert (P[2040, 37]['cpr'], P[2040, 37]['ppi'], P[2040, 37]['idle'], P[2040, 37]['blocks']) == (255, 1, 1, 37)
    p = P[2048, 3073]
    assert (p['cpr'], p['ppi'], p['idle'], p['blocks'], p['uncapped'], p['iters'], p['last_live']) == (256, 1, 0, 1024, 3073, 2, (1024, 1))
    Q = {c: R.launch('colsum', c[1], c[0]) for c in R.COLSUM_CASES}
    assert (Q[8, 1]['ppi'], Q[8, 1]['blocks'], Q[8, 1]['last_live']) == (1024, 1, (1, 0, 0, 0))
    assert (Q[40, 1000]['ppi'], Q[40, 1000]['idle'], Q[40, 1000]['blocks'], Q[40, 1000]['last_live']) == (204, 4, 5, (1000, 0, 0, 0))
    assert (Q[96, 198]['ppi'], Q[96, 198]['idle'], Q[96, 198]['blocks'], Q[96, 198]['last_live']) == (85, 4, 3, (198, 0, 0, 0))
    q = Q[96, 21761]
    assert (q['blocks'], q['uncapped'], q['stride'], q['iters'], q['last_live']) == (256, 257, 21760, 1, (21760, 1, 0, 0))
    q = Q[96, 87140]
    assert (q['blocks'], q['iters'], q['last_live']) == (256, 2, (100, 0, 0, 0)) and 87140 - 100 == 4 * q['stride']
    assert (Q[2040, 37]['cpr'], Q[2040, 37]['ppi'], Q[2040, 37]['idle'], Q[2040, 37]['blocks']) == (255, 4, 4, 10)
    q = Q[2048, 4101]
    assert (q['ppi'], q['blocks'], q['uncapped'], q['iters'], q['last_live']) == (4, 256, 1026, 2, (5, 0, 0, 0))
    T = {n8: R.launch('gdn_bwd_post', 8 * n8) for n8 in R.POST_N8}
    assert (T[1]['blocks'], T[257]['blocks'], T[2097153]['blocks'], T[2097153]['uncapped']) == (1, 2, 8192, 8193)
    assert (T[2097153]['trips'], T[2097153]['last_trip']) == (2, 1) and T[257]['trips'] == 1
    for N, C, H, W, cpad in R.LAYOUT_CASES:
        Y = R.launch('layout', N * H * W)
        if W == 838861:
            # one pixel past the cap: the thread that took pixel 0 of image 0 takes the last pixel of image N - 1 in its second trip
            assert (Y['blocks'], Y['uncapped'], Y['trips'], Y['last_trip']) == (16384, 16385, 2, 1) and N * H * W == 4194305
            assert cpad % 8 == (4 if cpad == 4 else 0)
        else:
            assert Y['trips'] == 1 and Y['blocks'] == -(-N * H * W // 256)
    assert [c[4] % 8 for c in R.LAYOUT_CASES] == [0, 4, 0, 4, 0] and R.LAYOUT_CASES[1][1] % 4 == 1 and R.LAYOUT_CASES[2][4] - R.LAYOUT_CASES[2][1] >= 8
    assert [R.launch('layout', N * H * W)['trips'] for N, C, H, W in R.LAYOUT_BACK_CASES] == [1, 2]


def test_mse_sum_partials_add_up_and_own_the_right_chunks():
    c = _case(R.make_loss_case, 257, 'random')
    p = R.mse_sum(c['x'], c['y'], 2)
    d = c['x'].double() - c['y'].double()
    assert abs(float(p.sum()) - float((d * d).sum())) <= 1e-12 * float((d * d).sum())
    assert abs(float(p[1]) - float((d[256 * 8:] ** 2).sum())) <= 1e-12 * float(p[1])          # workgroup 1: chunk 256 alone
    # a grid of 2 over 1 100 chunks: workgroup b owns the chunks i with (i mod 512) // 256 == b
    x, y = torch.randn(8800).double(), torch.randn(8800).double()
    p = R.mse_sum(x, y, 2)
    i = torch.arange(1100)
    for b in range(2):
        own = ((i % 512) // 256 == b).repeat_interleave(8)
        assert abs(float(p[b]) - float((((x - y) ** 2)[own]).sum())) <= 1e-12 * float(p[b])
    p32 = R.mse_sum(x.float(), y.float(), 2, torch.float32)
    assert p32.dtype == torch.float32 and float((p32.double() - R.mse_sum(x.float(), y.float(), 2)).abs().max()) < 1e-3


@pytest.mark.parametrize('inverse', [False, True])
def test_gdn_halves_against_autograd(inverse):
    g = torch.Generator().manual_seed(5)
    M, C = 37, 24
    x = torch.randn(M, C, generator=g, dtype=torch.float64).requires_grad_(True)
    with torch.no_grad():
        x[3, 5] = 0.0
    gy = torch.randn(M, C, generator=g, dtype=torch.float64)
    beta = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    gamma = torch.rand(C, C, generator=g, dtype=torch.float64) * 0.1
    norm = beta + x.abs() @ gamma.t()
    y = x * norm if inverse else x / norm
    y.backward(gy)
    pre = R.gdn_bwd_pre(gy, x, norm, inverse)
    t = pre['d_norm'] @ gamma                                    # gamma^T d_norm, exact float64
    dx = R.gdn_bwd_post(pre['dx_direct'], x, t)
    assert float((dx - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert float((pre['d_beta'] - beta.grad).abs().max()) <= 1e-12 * float(beta.grad.abs().max())
    assert float(R.sign(torch.tensor([0.0, -0.0, 2.0, -3.0])).abs().sum()) == 2.0
    # the float32 form states the same thing
    pre32 = R.gdn_bwd_pre(gy.float(), x.float(), norm.float(), inverse, torch.float32)
    assert float((pre32['d_norm'].double() - pre['d_norm']).abs().max()) <= 1e-5 * float(pre['d_norm'].abs().max())


@pytest.mark.parametrize('has_g,relu', R.MSE_VARIANTS)
def test_relu_bwd_mse_against_autograd(has_g, relu):
    c = _case(R.make_loss_case, 257, 'random')
    scale = float(torch.tensor(c['scale'], dtype=torch.float32))
    out_kept = c['out'].double()
    z = out_kept.clone().requires_grad_(True)          # the relu's input: where out > 0 it equals out, elsewhere any non-positive value
    o = torch.relu(z) if relu else z
    loss = scale * ((o - c['t'].double()) ** 2).sum()
    if has_g:
        loss = loss + (c['g'].double() * o).sum()
    loss.backward()
    got, sc = R.relu_bwd_mse(c['g'] if has_g else None, out_kept, c['t'], c['scale'], relu)
    assert float((got - z.grad).abs().max()) <= 1e-12 * float(z.grad.abs().max())
    if relu:
        assert bool((got[out_kept <= 0] == 0).all()) and 0.2 < float((out_kept > 0).double().mean()) < 0.8
    if not has_g:
        want = R.mse_grad(c['out'], c['t'], scale)
        assert torch.equal(R.relu_bwd_mse(None, c['out'], c['t'], c['scale'], False)[0], want)
    assert bool((sc >= got.abs() - 1e-12).all())
    a = R.relu_bwd(c['g'], c['out'], c['add'])
    assert torch.equal(a, torch.where(c['out'].double() > 0, c['g'].double() + c['add'].double(), torch.zeros((), dtype=torch.float64)))


def _is_bf16(t):
    return torch.equal(t.to(torch.bfloat16).double(), t.double())


@pytest.mark.parametrize('n8', R.LOSS_N8)
def test_dyadic_loss_operands_are_exact(n8):
    c = _case(R.make_loss_case, n8, 'dyadic')
    L = R.launch('loss', c['n'])
    for k in ('x', 'y', 'g', 'out', 't', 'add'):
        assert float(c[k].abs().max()) <= 4 and torch.equal(c[k], c[k].round())
    p = R.mse_sum(c['x'], c['y'], L['blocks'])                 # the terms are positive integers: the partial IS the sum of magnitudes
    assert float(p.max()) < 2 ** 24 and torch.equal(p, p.round())
    # the last ragged trip's chunks change their workgroup's partial
    first = (L['trips'] - 1) * L['blocks'] * 256
    d = (c['x'].double() - c['y'].double()).view(-1, 8)[first:]
    assert d.shape[0] == L['last_trip'] and float((d[-1] ** 2).sum()) > 0
    assert c['scale'] == 0.5
    for has_g, relu in R.MSE_VARIANTS:
        v, _ = R.relu_bwd_mse(c['g'] if has_g else None, c['out'], c['t'], c['scale'], relu)
        assert _is_bf16(v) and float(v.abs().max()) <= 12
    assert _is_bf16(R.mse_grad(c['x'], c['y'], 0.5)) and _is_bf16(R.relu_bwd(c['g'], c['out'], c['add']))
    for base in (0, c['n'] - 8):                                 # a `>= 0` mask would let these through
        assert float(c['out'][base]) == 0 and float(c['out'][base + 1]) == 0 and bool(torch.signbit(c['out'][base + 1]))
        assert bool((c['g'][base:base + 2] != 0).all()) and bool((c['g'][base:base + 2] + c['add'][base:base + 2] != 0).all())
        assert bool((c['g'][base:base + 2] - c['t'][base:base + 2] != 0).all())


@pytest.mark.parametrize('C,M', R.PRE_CASES)
def test_dyadic_gdn_pre_operands_are_exact(C, M):
    c = _case(R.make_pre_case, C, M, 'dyadic')
    assert float(c['gy'].abs().max()) <= 4 and float(c['x'].abs().max()) <= 4 and set(c['norm'].unique().tolist()) <= {1.0, 2.0}
    for inverse in (False, True):
        r = R.gdn_bwd_pre(c['gy'], c['x'], c['norm'], inverse)
        q = r['d_norm'] * 4                                      # unit 1 / 4
        assert torch.equal(q, q.round()) and float(r['d_beta_scale'].max()) * 4 < 2 ** 24
        assert _is_bf16(r['d_norm']) and _is_bf16(r['dx_direct'])
        assert bool((r['d_norm'][M - 1] != 0).all())             # the pixel the last ragged trip reaches counts in every column


@pytest.mark.parametrize('C,M', R.COLSUM_CASES)
def test_dyadic_colsum_operands_are_exact(C, M):
    c = _case(R.make_colsum_case, C, M, 'dyadic')
    s, sc = R.colsum(c['x'])
    assert float(c['x'].abs().max()) <= 8 and torch.equal(c['x'], c['x'].round()) and float(sc.max()) < 2 ** 24
    assert bool((c['x'][M - 1] != 0).all())


@pytest.mark.parametrize('n8', R.POST_N8)
def test_dyadic_post_operands_are_exact(n8):
    c = _case(R.make_post_case, n8, 'dyadic')
    assert _is_bf16(R.gdn_bwd_post(c['dx_direct'], c['x'], c['t']))
    for kind in R.KINDS[:1] if n8 > 257 else R.KINDS:
        c = _case(R.make_post_case, n8, kind)
        for base in (0, c['n'] - 8):
            x = c['x'][base:base + 4]
            assert x.tolist() == [0.0, 0.0, 2.0, -3.0] and bool(torch.signbit(x[1])) and not bool(torch.signbit(x[0]))
            assert bool((c['t'][base:base + 4] != 0).all())


def test_layout_reference_and_specials():
    sp = R.layout_specials()
    b = sp.to(torch.bfloat16).view(torch.int16).tolist()
    u = [v & 0xFFFF for v in b]
    assert u[:4] == [0x0000, 0x8000, 0x7F80, 0xFF80] and bool(torch.isnan(sp[4]))
    assert u[5:8] == [0x0000, 0x8080, 0x0080]                    # subnormals: to zero, and up to the smallest normal
    assert u[8:10] == [0x7F80, 0xFF80]                           # the largest finite f32 rounds to inf
    assert u[10:] == [0x3F80, 0x3F81, 0x3F80, 0x3F82, 0xBF82, 0x3F81, 0x3F82]   # below / above a tie, ties to even, around the odd tie
    x, pos = R.make_layout_case(2, 9, 3, 7)
    assert len(set(pos)) == len(pos) == 2 * len(sp) and pos[len(sp)] == (1, 8, 20)          # the last pixel among them
    y = R.nchw_to_nhwc_bf16(x, 12)
    assert y.shape == (2, 3, 7, 12) and bool((y[..., 9:] == 0).all())
    n, c, p = pos[3]
    assert float(y.view(2, 21, 12)[n, p, c]) == float('-inf')
    assert torch.equal(R.nhwc_bf16_to_nchw(y)[:, :9][~torch.isnan(x)], x.to(torch.bfloat16).float()[~torch.isnan(x)])


# ---- calibration ----

def _calibrate():
    if _measured:
        return _measured
    for n8 in R.LOSS_N8:
        _measured['loss', n8] = R.f32_error_loss(_case(R.make_loss_case, n8, 'random'))
    for C, M in R.PRE_CASES:
        _measured['pre', C, M] = R.f32_error_pre(_case(R.make_pre_case, C, M, 'random'))
    for C, M in R.COLSUM_CASES:
        _measured['colsum', C, M] = R.f32_error_colsum(_case(R.make_colsum_case, C, M, 'random'))
    return _measured


def test_float32_calibration():
    for key, e in _calibrate().items():
        print('calibration {}: '.format(key) + '  '.join('{} {:.2e}'.format(k, v) for k, v in e.items()))
        for k, v in e.items():
            assert v <= R.E_F32_MAX[k], (key, k, v, R.E_F32_MAX[k])


def test_float32_constants_are_the_measured_maxima():
    m = _calibrate()
    assert set(R.E_F32_MAX) == {'mse_sum', 'relu_bwd_mse', 'd_norm', 'dx_direct', 'd_beta', 'colsum'}
    for k, const in R.E_F32_MAX.items():
        worst = max(e[k] for e in m.values() if k in e)
        print('maximum {}: {:.3e} (constant {:.3e})'.format(k, worst, const))
        assert 0.9 * const <= worst <= const, k
    # what the GPU test's slack has to tell apart: a lost chunk, pixel or mask is an error of the order of the output itself
    assert R.F32_MARGIN == 8.0 and all(R.F32_MARGIN * v < 1e-5 for v in R.E_F32_MAX.values())
