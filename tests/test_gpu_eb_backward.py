"""-m gpu: sc2_eb_backward (and sc2_eb_forward on the same operands) against the float64 reference of tests/ref_eb.py, called
directly through hip.eb_backward / hip.eb_forward at every launch shape the launcher can choose.

The backward kernel is f32 end to end, so it is held to f32-grade bounds, not to the 6e-2 of the model-level gradient tests (bf16
convolutions in the same graph): a wrong slot among the 59 per-channel sums, a missing 1 - tanh^2 factor, a plane skipped or counted
twice by a workgroup that walks several images, a partial row left unzeroed are errors of 1e-2 and more.

  metrics  E_y = max |g_y - ref| / max |ref|;  E_p = max over channels of max_k |g_params[c, k] - ref[c, k]| / max_k |ref[c, k]|,
           k = 0..58; slots 59..63 exactly zero; in dequantize mode g_y exactly zero.
  bound    8 x the error of the float32 CPU evaluation of the same reference under the same metric (ref_eb.E_Y_F32_MAX / E_P_F32_MAX,
           measured by tests/test_eb_ref_cpu.py) -- never anything measured on the kernel.  The factor allows the device's tanhf / expf
           a few ulp where libm is within one, and the kernel's order of summation.
  cases    ref_eb.CASES: the smallest shapes that reach planes_per_wg 1 / 2 / 4 / 8 and one or two partial rows per plane; what the
           library reports (sc2_eb_backward_planes_per_wg, sc2_eb_bits_partial_len) must equal the table, so the coverage cannot rot.
           Both modes, upstream gradients g_yhat only / g_lik only / both, lik_bound 1e-9 and 0.0 on every case and 1e-2 on three
           (gate shut on a real share of the elements: asserted on the reference by tests/test_eb_ref_cpu.py and again here).
  inputs   decidable (ref_eb.make_decidable): no element within 1e-6 of a bound or 1e-4 of a rounding tie, so that a correct f32
           evaluation cannot legitimately take the other branch.
Measured kernel values: profiles/r17_gpu_eb_backward.log.
"""
import pytest
import torch

import ref_eb as E

pytestmark = pytest.mark.gpu

SHAPES = [c[0] for c in E.CASES]
BOUND_Y = E.F32_MARGIN * E.E_Y_F32_MAX
BOUND_P = E.F32_MARGIN * E.E_P_F32_MAX
_cache = {}


def _reference(S, R, shape):
    """The case's operands and, per mode, the float64 forward and every (bound, combination) gradient -- computed once, shared by
    the tests of the shape, never modified."""
    if shape not in _cache:
        case = E.make_case(S, R, shape)
        assert case['moved'] <= E.MAX_MOVED
        for mode in (E.NOISE, E.DEQUANTIZE):
            r = E.EbRef(case['P'], case['y'], case['noise'], mode)
            out = {'fwd': {b: r.forward(b) for b in E.bounds_of(shape)}, 'bwd': {}, 'open': {}}
            for b in E.bounds_of(shape):
                out['open'][b] = r.gate(b, case['g_lik'].double()).double().mean().item()
                for combo in E.COMBOS:
                    out['bwd'][b, combo] = r.backward(b, *E.upstream(case, combo))
            case[mode] = out
        _cache[shape] = case
    return _cache[shape]


def _to(dev, t):
    return None if t is None else t.to(dev).contiguous()


def test_launch_shapes_are_the_table(S, dev):
    lib = S.hip.lib()
    seen = set()
    for (N, C, HW), ppw, rows in E.CASES:
        assert lib.sc2_eb_backward_planes_per_wg(N, C, HW) == ppw, (N, C, HW)
        assert lib.sc2_eb_bits_partial_len(N, C, HW) == N * C * rows, (N, C, HW)
        assert rows == (HW + 1023) // 1024
        seen.add((ppw, 1 if rows == 1 else 2))
    assert {p for p, _ in seen} == {1, 2, 4, 8} and {r for _, r in seen} == {1, 2}
    assert seen == {(1, 1), (2, 1), (4, 1), (8, 1), (1, 2), (2, 2)}                    # as listed: > 1 plane AND > 1 row at once too
    assert lib.sc2_eb_backward_planes_per_wg(256, 24, 55 * 55) == 8                    # the stage-1 training step at bs 256
    assert lib.sc2_eb_backward_planes_per_wg(0, 24, 9) == 0
    gate = {c[0]: c[1] for c in E.CASES if c[0] in E.GATE_CASES}
    assert len(gate) == 3 and max(gate.values()) > 1


@pytest.mark.parametrize('mode', [E.NOISE, E.DEQUANTIZE], ids=['noise', 'dequantize'])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_eb_backward_kernel(S, R, dev, shape, mode):
    case = _reference(S, R, shape)
    ref = case[mode]
    P, y, noise = _to(dev, case['P']), _to(dev, case['y']), _to(dev, case['noise'])
    failures = []
    for bound in E.bounds_of(shape):
        if bound == E.BOUND_GATE:
            assert 0.05 <= ref['open'][bound] <= 0.95, 'gate open on {} of the elements'.format(ref['open'][bound])
        else:
            assert ref['open'][bound] == 1.0
        for combo in E.COMBOS:
            g_yhat, g_lik = (_to(dev, t) for t in E.upstream(case, combo))
            g_y, g_p = S.hip.eb_backward(y, P, mode, noise if mode == E.NOISE else None, g_yhat, g_lik, lik_bound=bound)
            g_y2, g_p2 = S.hip.eb_backward(y, P, mode, noise if mode == E.NOISE else None, g_yhat, g_lik, lik_bound=bound)
            assert torch.equal(g_y, g_y2) and torch.equal(g_p, g_p2), 'two calls on equal inputs differ'
            want_y, want_p = ref['bwd'][bound, combo]
            g_y, g_p = g_y.cpu(), g_p.cpu()
            assert g_p.shape == (shape[1], 64) and bool((g_p[:, E.N_SLOTS:] == 0).all()), 'slots 59..63 are not zero'
            if mode == E.DEQUANTIZE:
                assert bool((g_y == 0).all()), 'dequantize mode: g_y is not exactly zero'
            ey, ep = E.e_y(g_y, want_y), E.e_p(g_p[:, :E.N_SLOTS], want_p[:, :E.N_SLOTS])
            print('eb_backward {}x{}x{} {} bound {:g} {:5s}: E_y {:.3e} (bound {:.3e})  E_p {:.3e} (bound {:.3e})'.format(
                *shape, 'noise' if mode == E.NOISE else 'dequantize', bound, combo, ey, BOUND_Y, ep, BOUND_P))
            if not (ey <= BOUND_Y and ep <= BOUND_P):
                failures.append((bound, combo, ey, ep))
    assert not failures, 'beyond {:.3e} / {:.3e}: {}'.format(BOUND_Y, BOUND_P, failures)


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_eb_backward_partial_rows(S, R, dev, shape):
    """The layout the caller sums: on buffers poisoned with NaN every partial row and every g_y element is written, and only row 0 of
    the first plane of each workgroup carries sums (hip.eb_backward adds the rows up from torch.empty storage)."""
    case = _reference(S, R, shape)
    N, C, HW = shape
    hip, lib = S.hip, S.hip.lib()
    ppw, n_partial = lib.sc2_eb_backward_planes_per_wg(N, C, HW), lib.sc2_eb_bits_partial_len(N, C, HW)
    rows = n_partial // (N * C)
    P, y, noise = _to(dev, case['P']), _to(dev, case['y']), _to(dev, case['noise'])
    g_yhat, g_lik = _to(dev, case['g_yhat']), _to(dev, case['g_lik'])
    g_y = torch.full_like(y, float('nan'))
    part = torch.full((n_partial, 64), float('nan'), dtype=torch.float32, device=dev)
    args = (hip._ptr(y), hip._ptr(noise), hip._ptr(P), N, C, HW, E.NOISE, 1e-9, hip._ptr(g_yhat), hip._ptr(g_lik), hip._ptr(g_y),
            hip._ptr(part))
    assert lib.sc2_eb_backward(*args, n_partial + 1, hip._stream()) == -1        # a wrong row count is refused, nothing is launched
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(g_y).all())
    assert lib.sc2_eb_backward(*args, n_partial, hip._stream()) == 0
    assert not bool(torch.isnan(g_y).any()) and not bool(torch.isnan(part).any()), 'an output element was left unwritten'
    _, g_p = hip.eb_backward(y, P, E.NOISE, noise, g_yhat, g_lik, lik_bound=1e-9)
    assert torch.equal(part.view(N, C, rows, 64).sum(dim=(0, 2)), g_p)               # (the sum hip.eb_backward makes, on its rows)
    part = part.view(N, C, rows, 64).cpu()
    first = torch.zeros(N, C, rows, dtype=torch.bool)
    first[::ppw, :, 0] = True
    assert bool((part[~first] == 0).all()), 'a row other than the first of a workgroup is not zero'
    assert bool((part[first][:, :58].abs().amax(dim=1) > 0).all()) and bool((part[..., E.N_SLOTS:] == 0).all())


@pytest.mark.parametrize('mode', [E.NOISE, E.DEQUANTIZE], ids=['noise', 'dequantize'])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_eb_forward_kernel_on_the_same_inputs(S, R, dev, shape, mode):
    case = _reference(S, R, shape)
    N, C, HW = shape
    P, y, noise = _to(dev, case['P']), _to(dev, case['y']), _to(dev, case['noise'])
    # y_hat is two IEEE f32 operations: the CPU gives the same bits
    med = case['P'][:, 58].view(1, C, 1)
    y_hat_f32 = case['y'] + case['noise'] if mode == E.NOISE else torch.round(case['y'] - med) + med
    for bound in E.bounds_of(shape):
        want_y_hat, _, want_lik, want_bits = case[mode]['fwd'][bound]
        y_hat, nhwc, lik, bits = S.hip.eb_forward(y, P, mode, noise=noise if mode == E.NOISE else None, lik_bound=bound,
                                                  want_nhwc=True, want_bits=True)
        assert torch.equal(y_hat.cpu(), y_hat_f32)
        assert (y_hat_f32.double() - want_y_hat).abs().max().item() <= 2.0 ** -17           # one ulp at |y_hat| < 128
        torch.testing.assert_close(lik.cpu(), want_lik.float(), rtol=2e-4, atol=2e-7)
        assert bits.numel() == S.hip.lib().sc2_eb_bits_partial_len(N, C, HW) == N * C * ((HW + 1023) // 1024)
        total = want_bits.sum().item()
        assert abs(bits.double().sum().item() - total) <= 1e-4 * total
        assert nhwc.shape == (N, HW, C) and torch.equal(nhwc.cpu(), y_hat_f32.to(torch.bfloat16).permute(0, 2, 1))
        # per plane and tile: the partial sums are laid out (n, c, tile)
        rows = (HW + 1023) // 1024
        per_row = torch.stack([want_bits[..., r * 1024:(r + 1) * 1024].sum(dim=2) for r in range(rows)], dim=2)
        torch.testing.assert_close(bits.view(N, C, rows).cpu().double(), per_row, rtol=1e-3, atol=0.5)


def test_module_gradients_at_eight_planes_per_workgroup(S, R, dev):
    """S.EntropyBottleneck under autograd (autograd._EbFn + effective_params()) at 32 x 128 x 5, training mode with given noise,
    against the float64 oracle module: the gradients of matrices, biases, factors, quantiles and the input, under the kernel test's
    metrics and bound (a channel's 58 raw parameters + its three quantiles as one row)."""
    shape = (32, 128, 5)
    assert S.hip.lib().sc2_eb_backward_planes_per_wg(*shape) == 8
    case = _reference(S, R, shape)
    C = shape[1]
    ref = E.perturbed_oracle(R, C, 0)
    ref.load_state_dict(case['eb'].state_dict())
    ref = ref.double().train()
    yo = case['y'].double().clone().requires_grad_(True)
    y_hat, lik = ref(yo, noise=case['noise'].double().clone())
    ((y_hat * case['g_yhat'].double()).sum() + (lik * case['g_lik'].double()).sum()).backward()
    m = S.EntropyBottleneck(C)
    m.load_state_dict({k: v.clone() for k, v in case['eb'].state_dict().items()})
    m.to(dev).train()
    yd = case['y'].to(dev).requires_grad_(True)
    y_hat_d, lik_d = m(yd, noise=case['noise'].to(dev))
    assert y_hat_d.requires_grad and lik_d.requires_grad
    torch.testing.assert_close(lik_d.detach().cpu(), lik.detach().float(), rtol=2e-4, atol=2e-7)
    ((y_hat_d * case['g_yhat'].to(dev)).sum() + (lik_d * case['g_lik'].to(dev)).sum()).backward()

    def rows(mod):
        return torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().double().reshape(C, -1)
                          for _, p in mod.named_parameters()], dim=1)
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in ref.named_parameters()]
    got, want = rows(m), rows(ref)
    assert want.shape == (C, 61) and bool((want[:, :58].abs().amax(dim=1) > 0).all())
    ey, ep = E.e_y(yd.grad.cpu(), yo.grad), E.e_p(got, want)
    print('module 32x128x5 noise: E_y {:.3e} (bound {:.3e})  E_p {:.3e} (bound {:.3e})'.format(ey, BOUND_Y, ep, BOUND_P))
    assert ey <= BOUND_Y and ep <= BOUND_P
