"""CPU: tests/ref_bn.py -- the float64 reference tests/test_gpu_bn_train.py holds sc2_bn_train_fwd / sc2_bn_train_bwd against -- is
itself proved against torch, its case table is tied to the restated launcher arithmetic, and its float32 form is calibrated.

* reference against torch: the float64 form equals torch.native_batch_norm(training=True) + residual + ReLU and its autograd in
  float64 on the same operands within 1e-12 relative -- y, save_mean / save_rstd, both running statistics, dx, dgamma, dbeta and the
  residual's gradient (= the contract's dz) -- on every case and (relu, residual) combination, and with momentum 0.25 / eps 1e-3 on
  C = 24.  The contract's mask comes from the bf16 y, torch's from its own float64 output: they can differ only where the
  pre-activation is within 1e-9 of 0, and no case has such an element (asserted).  The single-pass and the two-pass variance agree in
  float64.
* case table: cpr, ppi, idle threads and nb of ref_bn.CASES equal ref_bn.launch(); the table reaches what it was chosen for (idle
  threads, a lone row past the last full trip, the unrolled loop of bn_sum_partials alone / followed by its tail, finalize workgroups
  with 8 and 24 live channels, nb at its cap, a second grid-stride trip of the stream kernels).
* inputs: bf16-representable, all channels different, channel 1 at mu = 4 sigma, channel 2 constant (variance exactly 0, rstd =
  1 / sqrt(eps) in both forms), exact zeros present, gamma of both signs.
* calibration: the float32 form (one pass, E[x^2] - mean^2, scale / shift and ca / cb / cc as csrc/bn.hip documents them; fixed
  pairwise order of summation, so the figures do not depend on the host) against the float64 form under the metrics of ref_bn.py,
  maximum over the four (relu, residual) combinations:

      C     M      mom   eps    y         dx        save_mean save_rstd run_mean  run_var   dbeta     dgamma
      8     2      0.1   1e-05  2.65e-08  5.09e-08  0.00e+00  6.77e-08  3.65e-08  1.11e-07  0.00e+00  9.06e-08
      24    1361   0.1   1e-05  4.59e-07  2.64e-07  8.02e-08  3.93e-07  7.00e-08  5.84e-08  5.21e-09  3.63e-08
      24    1361   0.25  0.001  6.12e-07  3.33e-07  8.02e-08  4.67e-07  6.15e-08  7.90e-08  5.21e-09  3.37e-08
      128   2049   0.1   1e-05  6.12e-07  4.59e-07  1.26e-07  6.94e-07  1.06e-07  9.47e-08  5.54e-09  7.24e-08
      40    19585  0.1   1e-05  5.51e-07  4.18e-07  7.08e-08  4.87e-07  8.97e-08  8.63e-08  1.58e-09  9.76e-09
      72    14337  0.1   1e-05  1.11e-06  6.08e-07  8.74e-08  1.08e-06  1.13e-07  6.88e-08  3.70e-09  2.97e-08
      1032  100    0.1   1e-05  4.20e-07  4.59e-07  8.37e-08  8.20e-07  1.10e-07  1.18e-07  1.18e-08  1.81e-07
      2040  37     0.1   1e-05  5.78e-07  5.96e-07  7.14e-08  9.30e-07  1.19e-07  9.96e-08  2.46e-08  5.85e-07
      2048  8200   0.1   1e-05  1.04e-06  7.58e-07  1.55e-07  1.04e-06  1.36e-07  1.13e-07  6.37e-09  6.69e-08

  The maxima, rounded up in the third digit, are ref_bn.E_F32_MAX.  All are a few units of 2^-24 = 6e-8 of the condition scale: save_rstd
  and y are largest where a channel's mean is several deviations (E[x^2] - mean^2 loses that factor squared), dbeta is small because
  the partial sums of N(0, 1) gradients stay far below sum |dz|.  The test re-measures every row, fails if a figure exceeds its constant and
  if a maximum falls below 0.9 x its constant (a constant that has come loose from what it measures).
"""
import pytest
import torch

import ref_bn as B

_cases = {}
_measured = {}


def _case(C, M):
    if (C, M) not in _cases:
        _cases[C, M] = B.make_case(C, M)
    return _cases[C, M]


def test_case_table_is_the_launcher_arithmetic():
    reach = {}
    for C, M, cpr, ppi, idle, nb in B.CASES:
        L = B.launch(M, C)
        assert (L['cpr'], L['ppi'], L['idle'], L['nb']) == (cpr, ppi, idle, nb), (C, M, L)
        assert L['chunks'] == M * C // 8 and L['ws_floats'] == nb * 2 * C + 3 * C
        assert nb == min(max(-(-M // (8 * ppi)), 1), 512)
        reach[C, M] = L
    assert reach[8, 2]['fin_blocks'] == 1 and reach[8, 2]['fin_live_last'] == 8                # 510 threads own no row
    L = reach[24, 1361]                                                                        # one row past the last full trip
    assert L['idle'] == 2 and 1361 - 1 == L['nb'] * L['ppi'] * B.BN_UNROLL * 2
    assert reach[128, 2049]['nb'] == 9 and reach[128, 2049]['unrolled_trips'] == 0 and reach[128, 2049]['tail_trips'] == 2
    assert (reach[40, 19585]['unrolled_trips'], reach[40, 19585]['tail_trips']) == (1, 0)      # smallest nb that enters the unrolled loop
    assert B.launch(19585 - 1, 40)['nb'] == 24 and B.launch(19585 - 1, 40)['unrolled_trips'] == 0
    assert (reach[72, 14337]['unrolled_trips'], reach[72, 14337]['tail_trips']) == (1, 1)      # unrolled loop THEN tail
    assert reach[1032, 100]['idle'] == 125 and reach[1032, 100]['fin_live_last'] == 8
    assert reach[2040, 37]['fin_blocks'] == 64 and reach[2040, 37]['fin_live_last'] == 24
    L = reach[2048, 8200]
    assert L['nb'] == 512 and -(-8200 // (8 * L['ppi'])) > 512 and (L['unrolled_trips'], L['tail_trips']) == (16, 0)
    assert L['chunks'] == 2099200 == B.STREAM_GRID_CAP * B.STREAM_THREADS + 2048 and L['stream_trips'] == 2
    assert all(reach[k]['stream_trips'] == 1 for k in reach if k != (2048, 8200))
    assert {L['idle'] > 0 for L in reach.values()} == {True, False}


@pytest.mark.parametrize('C,M', [c[:2] for c in B.CASES])
def test_inputs(C, M):
    c = _case(C, M)
    for k in ('x', 'residual', 'dy'):
        assert c[k].dtype == torch.float32 and c[k].shape == (M, C) and torch.equal(B.bf16(c[k]), c[k])
    x = c['x'].double()
    assert bool((x[:, 2] == 0.5).all())
    assert all(float(x[r, ch]) == 0.0 and ch != 2 for r, ch in c['zeros']) and len(set(c['zeros'])) >= min(5, M)
    assert bool((c['gamma'] > 0).any()) and bool((c['gamma'] < 0).any())
    assert bool((c['gamma'].abs() >= 0.5).all()) and bool((c['gamma'].abs() <= 1.5).all()) and bool((c['beta'].abs() <= 0.5).all())
    assert bool((c['running_var'] > 0).all()) and bool((c['running_mean'] != 0).all())
    r = B.BnRef(c['x'], c['gamma'], c['beta'], c['running_mean'], c['running_var'])
    # all channels differ in their statistics (and in gamma, beta): a channel mix-up changes every output
    # (sums of 100 bf16 values can coincide between two of 1032 channels: the pair (mean, rstd) is what has to differ)
    assert torch.unique(torch.stack([r.mean, r.rstd], 1), dim=0).shape[0] == C
    for t in (c['gamma'], c['beta']):
        assert torch.unique(t).numel() == C
    if M >= 1000:
        assert 3.5 <= float(r.mean[1] * r.rstd[1]) <= 4.5                                      # channel 1: mu = 4 sigma
    for dtype in (torch.float64, torch.float32):                                               # channel 2 is exact in both forms
        q = B.BnRef(c['x'], c['gamma'], c['beta'], dtype=dtype)
        assert float(q.mean[2]) == 0.5 and float(q.var[2]) == 0.0
        assert abs(float(q.rstd[2]) - 1e-5 ** -0.5) <= 1e-6 * 1e-5 ** -0.5


@pytest.mark.parametrize('C,M,momentum,eps', B.variants())
def test_reference_against_torch_in_float64(C, M, momentum, eps):
    c = _case(C, M)
    ref = B.BnRef(c['x'], c['gamma'], c['beta'], c['running_mean'], c['running_var'], momentum, eps)
    assert (ref.var - ref.var_single_pass).abs().max().item() <= 1e-12 * (ref.x * ref.x).mean(0).max().item()

    def close(got, want, what):
        scale = want.abs().max().item()
        assert (got - want).abs().max().item() <= 1e-12 * scale, (what, relu, res)
    for relu, res in B.COMBOS:
        x = c['x'].double().requires_grad_(True)
        g, b = c['gamma'].double().requires_grad_(True), c['beta'].double().requires_grad_(True)
        r = c['residual'].double().requires_grad_(True) if res else None
        rm, rv = c['running_mean'].double(), c['running_var'].double()
        z, save_mean, save_invstd = torch.native_batch_norm(x, g, b, rm, rv, True, momentum, eps)
        if res:
            z = z + r
        out = z.relu() if relu else z
        fwd = ref.forward(relu, c['residual'] if res else None)
        close(fwd['y'], out.detach(), 'y')
        close(fwd['mean'], save_mean, 'save_mean')
        close(fwd['rstd'], save_invstd, 'save_rstd')
        close(fwd['running_mean'], rm, 'running_mean')
        close(fwd['running_var'], rv, 'running_var')
        if relu:
            assert fwd['pre'].abs().min().item() > 1e-9, 'an element whose mask is undecidable'
        y = B.bf16(fwd['y']) if relu else None
        if relu:
            assert torch.equal(y > 0, out.detach() > 0)
        out.backward(c['dy'].double())
        bwd = ref.backward(c['dy'], y)
        close(bwd['dx'], x.grad, 'dx')
        close(bwd['dgamma'], g.grad, 'dgamma')
        close(bwd['dbeta'], b.grad, 'dbeta')
        if res:
            assert torch.equal(bwd['dz'], r.grad)
        if relu and M >= 100:
            share = (bwd['dz'] == 0).double().mean().item()
            assert 0.05 <= share <= 0.95, 'the mask is shut on {} of the elements'.format(share)


def test_the_mask_is_the_y_that_is_passed_in():
    c = _case(24, 1361)
    ref = B.BnRef(c['x'], c['gamma'], c['beta'])
    y = torch.where(torch.arange(1361 * 24).view(1361, 24) % 3 == 0, 1.0, -1.0)                # unrelated to any forward
    out = ref.backward(c['dy'], y)
    assert torch.equal(out['dz'], torch.where(y > 0, c['dy'].double(), torch.zeros((), dtype=torch.float64)))
    assert torch.equal(ref.backward(c['dy'], None)['dz'], c['dy'].double())


@pytest.mark.parametrize('C,M,momentum,eps', B.variants())
def test_float32_calibration(C, M, momentum, eps):
    e = B.f32_error(_case(C, M), momentum, eps)
    _measured[C, M, momentum] = e
    print('calibration C {} M {} momentum {} eps {}: '.format(C, M, momentum, eps) + '  '.join('{} {:.2e}'.format(k, v) for k, v in e.items()))
    for k, v in e.items():
        assert v <= B.E_F32_MAX[k], (k, v, B.E_F32_MAX[k])


def test_float32_constants_are_the_measured_maxima():
    for C, M, momentum, eps in B.variants():
        if (C, M, momentum) not in _measured:
            _measured[C, M, momentum] = B.f32_error(_case(C, M), momentum, eps)
    assert set(B.E_F32_MAX) == {'y', 'dx', 'save_mean', 'save_rstd', 'running_mean', 'running_var', 'dbeta', 'dgamma'}
    for k, const in B.E_F32_MAX.items():
        worst = max(e[k] for e in _measured.values())
        print('maximum {}: {:.3e} (constant {:.3e})'.format(k, worst, const))
        assert 0.9 * const <= worst <= const, k
    # what the GPU test's slack has to tell apart: a wrong row, chunk or mask is an error of the order of the output itself
    assert B.F32_MARGIN == 8.0 and all(B.F32_MARGIN * v < 1e-5 for v in B.E_F32_MAX.values())
