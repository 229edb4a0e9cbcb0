"""CPU: tests/ref_eb.py -- the float64 reference tests/test_gpu_eb_backward.py holds sc2_eb_backward / sc2_eb_forward against --
is itself proved against oracle.cpu_ref.EntropyBottleneck, its inputs are decidable, and its float32 form is calibrated.

* likelihoods: the reference on the float64 block of S.EntropyBottleneck.effective_params() (state loaded from the oracle) equals the
  oracle module cast to double within 1e-12, both modes, given noise -- the reading of the block's layout;
* gradients: the reference's block gradient chained through effective_params() equals the oracle's float64 autograd on `matrices`,
  `biases`, `factors`, `quantiles` and the input within 1e-10 relative, both modes, at likelihood bounds 1e-9 and 1e-2 (gate shut
  on a real share of elements) -- the softplus / tanh chain, the median slot and the LowerBound gate;
* decidability: make_decidable moves at most 1 % of the elements of every launch shape of the GPU test, and at lik_bound 1e-2 the gate
  is shut on >= 5 % and open on >= 5 % of the elements of the three cases that run it;
* calibration: the SAME reference evaluated in float32 on the CPU against its float64 form, under the GPU test's metrics E_y / E_p
  (ref_eb.e_y / e_p), maximum over modes, gradient combinations and bounds.  Measured (8 threads):

      N, C, HW          moved     E_y        E_p
      2, 24, 49         0.00043   3.85e-06   2.27e-05
      33, 32, 70        0.00026   3.01e-06   3.32e-05
      44, 24, 9         0.00011   5.61e-06   1.03e-04
      12, 192, 5        0.00009   1.78e-06   7.90e-05
      16, 128, 5        0.00020   3.25e-06   5.39e-05
      32, 128, 5        0.00020   2.69e-06   6.69e-05
      2, 6, 1089        0.00092   2.51e-06   1.84e-05
      8, 128, 1030      0.00029   2.22e-06   5.62e-05
      3, 5, 1025        0.00033   3.98e-06   6.32e-06

  The maxima are ref_eb.E_Y_F32_MAX / E_P_F32_MAX.  (E_y is above the 1e-7 of one f32 rounding because with the likelihood gradient
  alone d lik / d y is the difference of two nearly equal products, sigmoid' * L' at y_hat + 1/2 and at y_hat - 1/2: the density's
  slope, a tenth of either term.  E_p is largest where a channel has the fewest elements: 396 at 44 x 24 x 9.)  f32 sums depend on the
  thread count and the host's vector libm, so the test accepts a re-measured maximum between a quarter of and 1.25 x the constant.
"""
import copy

import pytest
import torch

import ref_eb as E

_cases = {}


def _case(S, R, shape):
    if shape not in _cases:
        _cases[shape] = E.make_case(S, R, shape)
    return _cases[shape]


def _modules(S, R, C, seed, bound):
    """(oracle module, package module with its state) both cast to double."""
    ref = E.perturbed_oracle(R, C, seed, likelihood_bound=bound)
    m = S.EntropyBottleneck(C, likelihood_bound=bound)
    m.load_state_dict({k: v.clone() for k, v in ref.state_dict().items()})
    return ref.double(), m.double()


def _inputs(N, C, HW, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(N, C, HW, generator=g) * torch.where(torch.rand(N, C, HW, generator=g) < 0.5, torch.tensor(24.0),
                                                           torch.tensor(4.0))).double()
    y[..., :6] = torch.tensor([150.0, -150.0, 400.0, -400.0, 1000.0, -1000.0], dtype=torch.float64)   # far tails: the 1e-9 bound engages
    noise = (torch.rand(N, C, HW, generator=g) - 0.5).double()
    return y, noise, torch.randn(N, C, HW, generator=g).double(), torch.randn(N, C, HW, generator=g).double()


@pytest.mark.parametrize('mode', [E.NOISE, E.DEQUANTIZE])
def test_likelihoods_match_the_oracle_in_float64(S, R, mode):
    N, C, HW = 3, 7, 41
    ref, m = _modules(S, R, C, 11, 1e-9)
    y, noise, _, _ = _inputs(N, C, HW, 12)
    with torch.no_grad():
        P = m.effective_params(torch.float64)
        assert P.dtype == torch.float64 and P.shape == (C, 64) and bool((P[:, 59:] == 0).all())
        want_y_hat, want_lik = ref(y, training=mode == E.NOISE, noise=noise if mode == E.NOISE else None)
    y_hat, raw, lik, bits = E.EbRef(P, y, noise, mode).forward(1e-9)
    assert (y_hat - want_y_hat).abs().max().item() <= 1e-12
    assert (lik - want_lik).abs().max().item() <= 1e-12
    assert bool((lik == raw.clamp_min(1e-9)).all()) and bool((lik == 1e-9).any()) and bool((lik > 1e-2).any())   # tails and bulk
    # (the oracle keeps its bound as an f32 buffer: 1e-9 rounded to f32 is 2.8e-8 relative away, 4e-8 in log2)
    assert torch.equal(bits, -torch.log2(lik)) and (bits + torch.log2(want_lik)).abs().max().item() <= 1e-7
    # and in f32 against the f32 oracle: the same layout reading at the kernel's precision
    ref32 = copy.deepcopy(ref).float()
    with torch.no_grad():
        _, lik32 = ref32(y.float(), training=mode == E.NOISE, noise=noise.float() if mode == E.NOISE else None)
    mine32 = E.EbRef(P.float(), y.float(), noise.float(), mode, torch.float32).forward(1e-9)[2]
    assert (mine32 - lik32).abs().max().item() <= 1e-6


@pytest.mark.parametrize('bound', [1e-9, 1e-2])
@pytest.mark.parametrize('mode', [E.NOISE, E.DEQUANTIZE])
def test_gradients_match_the_oracle_in_float64(S, R, mode, bound):
    N, C, HW = 3, 7, 41
    ref, m = _modules(S, R, C, 21, bound)
    y, noise, g_yhat, g_lik = _inputs(N, C, HW, 22)
    yo = y.clone().requires_grad_(True)
    y_hat, lik = ref(yo, training=mode == E.NOISE, noise=noise if mode == E.NOISE else None)
    ((y_hat * g_yhat).sum() + (lik * g_lik).sum()).backward()
    P = m.effective_params(torch.float64)
    r = E.EbRef(P, y, noise, mode)
    g_y, g_p = r.backward(bound, g_yhat, g_lik)
    if bound == 1e-2:
        shut = ~r.gate(bound, g_lik)
        assert 0.05 <= shut.double().mean().item() <= 0.95
    assert bool((g_p[:, 59:] == 0).all())
    P.backward(g_p)
    if mode == E.DEQUANTIZE:
        assert bool((g_y == 0).all()) and yo.grad is not None and bool((yo.grad == 0).all())
        assert bool((g_p[:, 58] != 0).all())                                        # d y_hat summed into the median's slot
    else:
        assert (g_y - yo.grad).abs().max().item() <= 1e-10 * yo.grad.abs().max().item()
    names = []
    for (name, want), (_, got) in zip(ref.named_parameters(), m.named_parameters()):
        gw = torch.zeros_like(want) if want.grad is None else want.grad
        gg = torch.zeros_like(got) if got.grad is None else got.grad
        scale = gw.abs().max().item()
        assert (gg - gw).abs().max().item() <= 1e-10 * scale, name
        names.append(name.split('.')[0])
        if name != 'quantiles' or mode == E.DEQUANTIZE:
            assert scale > 0, name
    assert sorted(set(names)) == ['biases', 'factors', 'matrices', 'quantiles'] and len(names) == 15


def test_float64_copies_do_not_share_gradients():
    """The conversion gotcha: two references built from the same float64 tensors are independent graphs."""
    P = torch.rand(2, 64, dtype=torch.float64)
    y = torch.randn(1, 2, 5, dtype=torch.float64)
    a, b = E.EbRef(P, y, torch.zeros_like(y), E.NOISE), E.EbRef(P, y, torch.zeros_like(y), E.NOISE)
    assert a.P is not P and a.P.data_ptr() != b.P.data_ptr() and a.y.data_ptr() != y.data_ptr()
    g = torch.ones_like(y)
    first = a.backward(0.0, g, g)
    again = a.backward(0.0, g, g)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]) and P.grad is None and y.grad is None


@pytest.mark.parametrize('shape', [c[0] for c in E.CASES])
def test_inputs_are_decidable(S, R, shape):
    c = _case(S, R, shape)
    assert c['moved'] <= E.MAX_MOVED, 'make_decidable moved {:.4%} of the elements'.format(c['moved'])
    for t in (c['P'], c['y'], c['noise'], c['g_yhat'], c['g_lik']):
        assert t.dtype == torch.float32
    assert not bool(E.undecidable(c['P'], c['y'], c['noise'], E.bounds_of(shape)).any())
    if shape in E.GATE_CASES:
        for mode in (E.NOISE, E.DEQUANTIZE):
            open_ = E.EbRef(c['P'], c['y'], c['noise'], mode).gate(E.BOUND_GATE, c['g_lik'].double()).double().mean().item()
            assert 0.05 <= open_ <= 0.95, 'gate open on {:.3f} of the elements'.format(open_)


def test_gate_cases_reach_several_planes_per_workgroup():
    table = {c[0]: c[1:] for c in E.CASES}
    assert len(E.GATE_CASES) == 3 and any(table[s][0] > 1 for s in E.GATE_CASES)
    assert {(p, min(r, 2)) for _, p, r in E.CASES} >= {(1, 1), (2, 1), (4, 1), (8, 1), (1, 2), (2, 2)}


def test_float32_calibration(S, R):
    worst_y = worst_p = 0.0
    for shape, _, _ in E.CASES:
        ey, ep = E.f32_error(_case(S, R, shape), shape)
        print('calibration N, C, HW = {}: moved {:.5f}  E_y {:.3e}  E_p {:.3e}'.format(shape, _case(S, R, shape)['moved'], ey, ep))
        worst_y, worst_p = max(worst_y, ey), max(worst_p, ep)
    print('maxima: E_y {:.3e}  E_p {:.3e}'.format(worst_y, worst_p))
    assert 0.25 * E.E_Y_F32_MAX <= worst_y <= 1.25 * E.E_Y_F32_MAX
    assert 0.25 * E.E_P_F32_MAX <= worst_p <= 1.25 * E.E_P_F32_MAX
    # what the GPU test's bound has to tell apart: the faults it exists for are errors of 1e-2 and more
    assert E.F32_MARGIN == 8.0 and E.F32_MARGIN * E.E_Y_F32_MAX < 1e-3 and E.F32_MARGIN * E.E_P_F32_MAX < 1e-2 / 8
