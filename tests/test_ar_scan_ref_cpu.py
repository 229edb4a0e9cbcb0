"""The sequential reference of the context-model scan (tests/ref_ar_scan.py) checked on the CPU before the kernel is held to it
(tests/test_gpu_ar_scan.py): it reproduces the established restatement of the model (tests/ref_input_hyperprior.py) through the
packing the header documents, its operand builders meet their preconditions at every shape the GPU test runs, and each
deliberately wrong step ('mutant') fails the very assertion the kernel is held to."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_ar_scan as RA  # noqa: E402
import ref_input_hyperprior as RH  # noqa: E402

EXACT_SHAPES = RA.SMALL_SHAPES + RA.WIDE_SHAPES + [RA.MANY_IMAGES[:5] + (RA.MANY_DISTINCT,)]


def _pack(r):
    """The restatement's weights in the packing of sc2_ar_scan_args (as JointAutoregressiveHierarchicalPriors._packed)."""
    M = r.M
    ep, cp = r.entropy_parameters, r.context_prediction
    w1 = ep[0].weight.detach().double()[:, :, 0, 0].numpy()           # [C1, 4M]: params first, then the context
    w2 = ep[2].weight.detach().double()[:, :, 0, 0].numpy()           # [C2, C1]
    w3 = ep[4].weight.detach().double()[:, :, 0, 0].numpy()           # [2M, C2]
    C1, C2 = w1.shape[0], w2.shape[0]
    C1p, C2p = (C1 + 7) // 8 * 8, (C2 + 7) // 8 * 8
    mw = (cp.weight * cp.mask).detach().double().numpy()              # [2M, M, 5, 5]
    taps = [(ky, kx) for ky in range(2) for kx in range(5)] + [(2, 0), (2, 1)]
    weights = {'wc': np.concatenate([mw[:, :, ky, kx].T for ky, kx in taps], 0), 'bc': cp.bias.detach().double().numpy(),
               'w1': np.zeros((2 * M, C1p)), 'w2': np.zeros((C1p, C2p)), 'b2': np.zeros(C2p),
               'w3': np.zeros((C2p, 2 * M)), 'b3': ep[4].bias.detach().double().numpy()}
    weights['w1'][:, :C1] = w1[:, 2 * M:].T
    weights['w2'][:C1, :C2] = w2.T
    weights['b2'][:C2] = ep[2].bias.detach().double().numpy()
    weights['w3'][:C2] = w3.T
    return weights, w1[:, :2 * M], ep[0].bias.detach().double().numpy(), C1p


def test_scan_ref_reproduces_the_restated_model():
    """Tap order, mask, packing convention: scan_ref on the packed weights of a float64 JointAutoregressiveHierarchicalPriors
    gives that model's compress_ar symbols and indexes, and its parallel gaussian_params(params, y_hat) to 1e-10."""
    torch.manual_seed(0)
    r = RH.JointAutoregressiveHierarchicalPriors(N=4, M=6).eval()
    with torch.no_grad():
        for mod in list(r.entropy_parameters) + [r.context_prediction]:
            if hasattr(mod, 'weight'):
                fan_in = mod.weight[0].numel()
                mod.weight.copy_(torch.randn_like(mod.weight) / math.sqrt(fan_in))
                mod.bias.copy_(torch.randn_like(mod.bias))
        r.entropy_parameters[4].weight.mul_(4.0)       # scales over many table rows
    for mod in r.entropy_parameters:
        if isinstance(mod, torch.nn.LeakyReLU):
            mod.negative_slope = RA.SLOPE              # the kernel's constant is the f32 nearest 0.01, 2e-8 from the double
    r.update()
    r.double()
    M, B, H, W = 6, 2, 4, 5
    g = torch.Generator().manual_seed(1)
    y = (8 * torch.randn(B, M, H, W, generator=g)).float().double()
    params = torch.randn(B, 2 * M, H, W, generator=g).float().double()
    weights, w1a, b1, C1p = _pack(r)
    p1 = np.zeros((B, H, W, C1p))
    p1[..., :w1a.shape[0]] = np.einsum('bkhw,nk->bhwn', params.numpy(), w1a) + b1
    gc = r.gaussian_conditional
    ref = RA.scan_ref(weights, p1, y.numpy(), gc.scale_table.numpy(), float(gc.lower_bound_scale.bound))
    with torch.no_grad():
        _, syms, idxs, y_hat = r.compress_ar(y, params)
        y_hat_ref = torch.from_numpy(ref['y_hat_pad'][:, 2:, 2:W + 2, :]).permute(0, 3, 1, 2).contiguous()
        par = r.gaussian_params(params, y_hat_ref)                                   # [B, 2M, H, W]
    assert np.array_equal(ref['symbols'], syms.numpy())
    assert np.array_equal(ref['indexes'], idxs.numpy())
    assert len(np.unique(ref['indexes'])) >= 6 and np.abs(ref['symbols']).max() >= 4
    assert torch.allclose(y_hat.float(), y_hat_ref.float(), rtol=0, atol=1e-5)
    par = par.permute(0, 2, 3, 1).reshape(B, H * W, 2 * M).numpy()
    assert np.abs(ref['gaussian_params'] - par).max() <= 1e-10 * np.abs(par).max()
    tf = RA.teacher_forced_ref(weights, p1, ref['y_hat_pad'])
    assert np.abs(tf['gaussian_params'] - par).max() <= 1e-10 * np.abs(par).max()


@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_exact_builder_preconditions(shape):
    case, ref = RA.cached('exact', shape)
    figures = RA.check_exact_preconditions(case, ref)
    print(shape, figures)
    RA.assert_exact(ref, ref)
    RA.assert_exact({k: RA.f32(v) if v.dtype == np.float64 else v for k, v in ref.items()}, ref)


@pytest.mark.parametrize('shape', RA.SMALL_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_random_builder_preconditions_and_bound(shape):
    """Both LeakyReLU branches occur; the float64 scan and an f32 evaluation of it (numpy's summation order) lie within the bound."""
    case, ref = RA.cached('random', shape)
    print(shape, RA.check_random_preconditions(case, ref))
    for name in ('wc', 'w1', 'w2', 'w3'):
        assert np.array_equal(RA.bf16_round(case['weights'][name]), case['weights'][name])
    assert RA.assert_random(case, ref) < 1e-6
    r32 = RA.scan_ref(case['weights'], case['p1'], case['y'], case['scale_table'], case['scale_bound'], dtype=np.float32)
    ratio = RA.assert_random(case, r32)
    print('f32 evaluation: largest |err| / bound = {:.3g}'.format(ratio))
    assert 0 < ratio < 1


def test_pixel_ranges_of_the_reference_compose():
    case, ref = RA.cached('exact', RA.SMALL_SHAPES[0])
    H, W = case['shape'][3:5]
    pad, parts = None, []
    for pix in [(0, 1), (1, 1), (1, W + 2), (W + 2, H * W)]:
        out = RA.scan_ref(case['weights'], case['p1'], case['y'], case['scale_table'], case['scale_bound'], pix=pix, y_hat_pad=pad)
        pad = out['y_hat_pad']
        parts.append(out)
    assert np.array_equal(pad, ref['y_hat_pad'])
    assert np.array_equal(sum(o['symbols'] for o in parts), ref['symbols'])
    assert np.array_equal(sum(o['gaussian_params'] for o in parts), ref['gaussian_params'])


# which assertion catches which mutant: the exact set never takes the leaky branch; a strict `<` changes only indexes and
# round-half-away only exact ties, which the random set meets with probability ~ 0
EXACT_CATCHES = [m for m in RA.MUTANTS if m != 'slope0']
RANDOM_CATCHES = [m for m in RA.MUTANTS if m not in ('lt', 'half_away')]
MUTANT_SHAPES = RA.SMALL_SHAPES[:2]       # the baseline and the K = 10 -> 3, 3, 3, 1 split


def _mutated(kind, shape, mutant):
    case, _ = RA.cached(kind, shape)
    return case, RA.scan_ref(case['weights'], case['p1'], case['y'], case['scale_table'], case['scale_bound'], mutant=mutant)


@pytest.mark.parametrize('shape', MUTANT_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('mutant', EXACT_CATCHES)
def test_mutant_fails_bit_equality_on_the_exact_set(mutant, shape):
    _, ref = RA.cached('exact', shape)
    _, mut = _mutated('exact', shape, mutant)
    with pytest.raises(AssertionError):
        RA.assert_exact(mut, ref)
    if mutant != 'lt':                    # ... and through gaussian_params alone (the strict search changes only indexes)
        assert not np.array_equal(mut['gaussian_params'], ref['gaussian_params'])


@pytest.mark.parametrize('shape', MUTANT_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('mutant', RANDOM_CATCHES)
def test_mutant_fails_the_running_bound_on_the_random_set(mutant, shape):
    case, mut = _mutated('random', shape, mutant)
    with pytest.raises(AssertionError, match='outside the bound'):
        RA.assert_random(case, mut)


def test_leaky_slope_is_invisible_to_the_exact_set():
    """Why the random set exists: with every pre-activation positive the slope-0 mutant equals the reference."""
    shape = RA.SMALL_SHAPES[0]
    RA.assert_exact(_mutated('exact', shape, 'slope0')[1], RA.cached('exact', shape)[1])
