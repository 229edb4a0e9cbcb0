"""The integer-operand helper (tests/exact_ints.py) itself, without a GPU: its f32 and f64 references against an int64 einsum, the
narrow operand rule at the K values the GPU cases use, the exactness bound, the one rounding of `cast`, the failure report of
`assert_bits_equal`, and the guard-band arena."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import exact_ints as E  # noqa: E402


@pytest.mark.parametrize('kind', ['wide', 'narrow'])
@pytest.mark.parametrize('cin,cout,k,stride,pad,dil,H,W,N', [(8, 16, 3, 1, 1, 1, 7, 9, 2), (16, 8, 5, 2, 2, 1, 11, 10, 1),
                                                             (32, 24, 1, 2, 0, 1, 5, 5, 3), (8, 8, 3, 1, 2, 2, 9, 8, 2),
                                                             (48, 24, 2, 1, 0, 1, 6, 4, 2), (8, 8, 3, 1, 1, 1, 1, 1, 1)])
def test_references_agree_with_int64_einsum(kind, cin, cout, k, stride, pad, dil, H, W, N):
    g = E.gen(cin, cout, k, H)
    K = cin * k * k
    x = E.operand(kind, (N, cin, H, W), K, g)
    w = E.operand(kind, (cout, cin, k, k), K, g)
    E.check_bound(K, x, w)
    want = E.conv_ref_int(x, w, stride, pad, dil)
    r64 = E.conv_ref(x, w, stride, pad, dil)
    r32 = E.conv_ref_f32(x, w, stride, pad, dil)
    assert r64.dtype == torch.float64 and torch.equal(r64.to(torch.int64), want) and torch.equal(r64, want.double())
    assert torch.equal(r32.double(), r64)
    assert torch.equal(E.cast(r64, torch.float32), r32)


@pytest.mark.parametrize('stride,pad,k,H,W', [(1, 1, 3, 6, 7), (2, 1, 3, 9, 10), (2, 0, 1, 7, 7), (2, 2, 5, 12, 11), (1, 0, 2, 5, 5)])
def test_gradient_references_agree_with_autograd_of_the_integer_conv(stride, pad, k, H, W):
    g = E.gen(stride, pad, k, H)
    cin, cout, N = 8, 16, 2
    x = E.wide((N, cin, H, W), g)
    w = E.wide((cout, cin, k, k), g)
    y = E.conv_ref(x, w, stride, pad)
    gy = E.wide(tuple(y.shape), g)
    xg = x.double().requires_grad_()
    wg = w.double().requires_grad_()
    torch.nn.functional.conv2d(xg, wg, None, stride, pad).backward(gy.double())
    assert torch.equal(E.dgrad_ref(gy, w, stride, pad, (H, W)), xg.grad)
    assert torch.equal(E.wgrad_ref(x, gy, k, k, stride, pad), wg.grad)
    assert torch.equal(E.wgrad_ref(-x.abs(), gy, k, k, stride, pad, x_abs=True), E.wgrad_ref(x.abs(), gy, k, k, stride, pad))
    assert torch.equal(xg.grad, xg.grad.round()) and torch.equal(wg.grad, wg.grad.round())


@pytest.mark.parametrize('K', [64, 1024, 2048, 4608, 9408])
def test_narrow_rule_keeps_outputs_bf16_exact(K):
    """K p_x p_w <= 1024 -> std <= 32; 4096 outputs per K stay within 256 (8 sigma), so each is a bf16-exact integer."""
    g = E.gen(K)
    p = E.narrow_p(K)
    assert K * p * p <= 1024 * 1.0000001 or p == 0.75 and K * p * p <= 1024
    x = E.narrow((64, K), K, g)
    w = E.narrow((64, K), K, g)
    assert set(torch.unique(x).tolist()) <= {-1.0, 0.0, 1.0} and (x == 0).any() and (x != 0).any()
    E.check_bound(K, x, w)
    ref = x.double() @ w.double().t()
    E.check_narrow(ref)
    assert ref.std().item() <= 32.0 * 1.1
    assert ref.abs().max().item() >= 8          # (the outputs are not trivially small either)
    assert torch.equal(E.cast(ref, torch.bfloat16).double(), ref)
    with pytest.raises(AssertionError):
        E.check_narrow(ref * 300)


def test_wide_outputs_exercise_the_bf16_rounding_and_its_ties():
    """512 -> 256 channels, 3x3 (K = 4608): the f32 conv equals the f64 one, the outputs run into the hundreds, a good share of
    them changes under the bf16 store and exact round-to-even ties (odd integers in 256..512) occur."""
    g = E.gen(4608)
    x = E.wide((1, 512, 10, 10), g)
    w = E.wide((256, 512, 3, 3), g)
    E.check_bound(4608, x, w, E.bias_ints(256, g), E.residual_ints((4,), g))
    r64 = E.conv_ref(x, w, 1, 1)
    assert torch.equal(E.conv_ref_f32(x, w, 1, 1).double(), r64)
    assert r64.abs().max().item() <= 9 * 4608 and r64.abs().max().item() > 512
    b = E.cast(r64, torch.bfloat16).double()
    assert 0.05 < (b != r64).double().mean().item() < 0.5
    a = r64.abs()
    assert int(((a > 256) & (a < 512) & (a % 2 == 1)).sum()) > 100
    trunc = (r64.float().view(torch.int32) & -65536).view(torch.float32).double()       # the store a truncating kernel would make
    assert (trunc != b).any()


def test_symbol_ties_are_met():
    """Medians that are multiples of 0.25 do produce exact .5 ties on integer outputs, so round-half-to-even is what the symbol cases
    of the GPU file pin (the operands of its 16 -> 40, 3x3 generic case)."""
    g = E.gen(16, 40, 3, 3, 7, 50, 3, 0, True)
    x, w = E.wide((3, 16, 7, 50), g), E.wide((40, 16, 3, 3), g)
    E.bias_ints(40, g)
    med = E.quarter_medians(40, g)
    d = E.conv_ref(x, w, 1, 1) - med.double().view(1, -1, 1, 1)
    ties = (d - torch.floor(d)) == 0.5
    assert int(ties.sum()) > 100
    r = torch.round(d[ties])
    assert torch.equal(r % 2, torch.zeros_like(r))          # torch.round is half-to-even, as rintf


def test_bound_and_integer_checks_refuse():
    g = E.gen(1)
    x, w = E.wide((4, 4), g), E.wide((4, 4), g)
    with pytest.raises(AssertionError):
        E.check_bound(1 << 22, x + 4.0 * (x == 0), w + 4.0 * (w == 0))
    with pytest.raises(AssertionError):
        E.check_bound(16, x * 0.5 + 0.25, w)
    with pytest.raises(AssertionError):
        E.check_bound(16, x + 257.0, w)          # 257 + small: not bf16 exact
    with pytest.raises(AssertionError):
        E.cast(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), torch.bfloat16)
    m = E.quarter_medians(32, g)
    assert torch.equal(m * 4, (m * 4).round()) and m.abs().max().item() <= 2


def test_assert_bits_equal_points_at_the_mismatch():
    ref = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).reshape(2, 3, 4, 8).to(torch.bfloat16)
    E.assert_bits_equal(ref.clone(), ref, 'same')
    got = ref.clone()
    got[1, 2, 1:3, 4:8] += 1
    with pytest.raises(AssertionError) as e:
        E.assert_bits_equal(got, ref, 'row')
    text = str(e.value)
    assert '8 of 192 elements differ' in text and 'first at (n, oh, ow, c) = (1, 2, 1, 4)' in text
    assert 'ONE output row' in text and 'ow in 1..2' in text and 'c//4 = 1' in text
    got = ref.clone()
    got[0, 0, 0, 0] = float('nan')
    with pytest.raises(AssertionError) as e:
        E.assert_bits_equal(got, ref, 'nan')
    assert '1 NaN' in str(e.value)
    with pytest.raises(AssertionError) as e:      # NCHW tensors are reported in (n, oh, ow, c) too
        E.assert_bits_equal(E.nchw(ref) + (torch.arange(8).view(1, 8, 1, 1) == 5), E.nchw(ref), 'channel', layout='nchw')
    assert 'c = 5' in str(e.value) and 'ONE' not in str(e.value)
    with pytest.raises(AssertionError):
        E.assert_bits_equal(ref.float(), ref, 'dtype')
    with pytest.raises(AssertionError) as e:
        E.assert_bits_equal(torch.zeros(3, 5), torch.ones(3, 5), '2-d')
    assert 'd1 in 0..4' in str(e.value)


def test_assert_bits_in_points_at_the_element_that_matches_no_candidate():
    a = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).reshape(2, 3, 4, 8).to(torch.bfloat16)
    b = a.clone()
    b[1, 0, 2, 5] += 1
    got = a.clone()
    got[1, 0, 2, 5] = b[1, 0, 2, 5]
    E.assert_bits_in(a, [a], 'one')
    E.assert_bits_in(got, [a, b], 'either')           # element-wise: some elements from one candidate, some from the other
    with pytest.raises(AssertionError) as e:
        E.assert_bits_in(got, [a], 'only a')
    assert '1 of 192 elements match none of the 1' in str(e.value) and '(n, oh, ow, c) = (1, 0, 2, 5)' in str(e.value)
    got[0, 1, 1, 1] = float('nan')
    with pytest.raises(AssertionError) as e:
        E.assert_bits_in(got, [a, b], 'nan')
    assert '(0, 1, 1, 1)' in str(e.value)
    with pytest.raises(AssertionError) as e:
        E.assert_bits_in(E.nchw(got), [E.nchw(a), E.nchw(b)], 'nchw', layout='nchw')
    assert '(0, 1, 1, 1)' in str(e.value)
    with pytest.raises(AssertionError):
        E.assert_bits_in(a.float(), [a], 'dtype')
    with pytest.raises(AssertionError):
        E.assert_bits_in(a, [], 'nothing admissible')


# --------------------------------------------------------------------------------------------- #
# GDN1 with a live gamma: what the GPU file's comparisons can see, proved on the references alone for the cases it runs
# --------------------------------------------------------------------------------------------- #
import test_gpu_exact_conv as G  # noqa: E402      (module import: its tests are not collected here; it needs no GPU to import)

DISCRIMINATION_FLOOR = 0.05       # share of the non-zero f32 outputs on which t * (1 / n) and the correctly rounded t / n differ
AMBIGUITY_CAP_WIDE = 1e-3         # share of a case's elements with more than one admissible bf16 value under a 1-ulp reciprocal
BF16, F32 = torch.bfloat16, torch.float32


def test_live_gamma_and_the_family_table():
    for C in (20, 32, 40, 48, 64, 96, 256, 512):
        g = E.gen(C)
        gamma = E.live_gamma(C, g)
        assert tuple(gamma.shape) == (C, C) and set(torch.unique(gamma).tolist()) <= {0.0, 0.5, 1.0, 2.0}
        assert bool(((gamma != 0).sum(0) == 3).all()) and bool(((gamma != 0).sum(1) == 3).all())
        assert torch.equal(gamma.to(BF16).float(), gamma)
        for kind in ('wide', 'narrow'):
            for inverse in (False, True):
                params = E.gdn_params(kind, C, g, inverse)
                assert [v[2] for v in params] == ['gamma 0 beta 1', 'gamma 0 beta 2', 'live gamma']
                beta = params[2][1]
                assert set(torch.unique(beta).tolist()) <= {1.0, 2.0, 3.0} and int((params[2][0] != 0).sum()) == 3 * C
    with pytest.raises(AssertionError):
        E.gdn_params('wide', 48, E.gen(1), False, tmax=float(1 << 22))
    assert set(G.GDN_TESTS) == {n for n in dir(G) if n.startswith('test_') and ('gdn' in n or 'first_stage' in n)}
    for name, (family, cases, geom) in G.GDN_TESTS.items():
        assert family in G.GDN_FAMILIES and len(cases) > 0
    for t_gemm, t_prod, rcp in G.GDN_FAMILIES.values():
        assert t_gemm in (BF16, F32) and t_prod in (BF16, F32) and rcp in ('ieee', 'rcpf')


def test_gdn_restate_is_the_documented_arithmetic():
    """Against f64 on a case small enough to read: forward = ONE rounding of t * fl(1 / n) (so within an ulp of, but not always
    equal to, fl(t / n)); inverse with integer operands below 2^24: exact.  The norm refuses what is not exact."""
    g = E.gen(7)
    t = torch.randint(-4000, 4001, (2, 48, 3, 5), generator=g).double()
    gamma, beta = E.live_gamma(48, g), torch.randint(1, 4, (48,), generator=g).float()
    n = E.gdn_norm(t, gamma, beta, F32)
    n64 = torch.einsum('oc,nchw->nohw', gamma.double(), t.abs()) + beta.double().view(1, -1, 1, 1)
    assert n.dtype == F32 and torch.equal(n.double(), n64)
    y = E.gdn_restate(t, gamma, beta, False, F32, F32, F32)
    r = (1.0 / n64).float()                                     # f64 quotient rounded to f32: the correctly rounded reciprocal
    assert torch.equal(y.double(), (t * r.double()).float().double())      # (t r is exact in f64: 12 + 24 bits)
    q = (t / n64).float()
    assert (y != q).any() and float(((y - q).abs() / q.abs().clamp_min(1e-30)).max()) < 2.0 ** -22
    yi = E.gdn_restate(t, gamma, beta, True, F32, F32, F32)
    assert torch.equal(yi.double(), (t * n64).float().double())
    tb = t.float().to(BF16).double()
    assert (tb != t).any()
    assert torch.equal(E.gdn_restate(t, gamma, beta, False, BF16, BF16, BF16), E.gdn_restate(tb, gamma, beta, False, F32, F32, BF16))
    assert torch.equal(E.gdn_norm(t, gamma, beta, BF16), E.gdn_norm(tb, gamma, beta, F32))
    with pytest.raises(AssertionError):
        E.gdn_norm(t, gamma * 0.3, beta, F32)
    with pytest.raises(AssertionError):
        E.gdn_norm(t * 4096, gamma, beta, F32)
    with pytest.raises(AssertionError):
        E.gdn_norm(t, gamma, beta * 0, F32)
    cands, many = E.gdn_admissible(t, gamma, beta, BF16, F32)
    assert len(cands) == 3 and all(c.dtype == BF16 for c in cands) and torch.equal(cands[0], E.gdn_restate(t, gamma, beta, False, BF16, F32, BF16))
    assert float(many.double().mean()) < 0.01


def _other(dtype):
    return BF16 if dtype == F32 else F32


def _count(a, b):
    return int(((a != b) | (torch.isnan(a) != torch.isnan(b))).sum())


@pytest.mark.parametrize('kind', ['wide', 'narrow'])
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('test', sorted(G.GDN_TESTS))
def test_gdn_cases_discriminate(test, kind, inverse, capsys):
    """For every case the GPU test `test` runs at (kind, inverse), on the live gamma: exactness of the norm (and, on the narrow set,
    of |t| in bf16; in the precise family, of the two-part bf16 split of |t|), the share of f32 outputs that tell t * (1 / n) from
    t / n, the share of elements with more than one admissible value under a 1-ulp reciprocal, and the number of elements each
    mutant of the restatement changes in the output types the GPU test compares.  One line per case is printed (-s shows it)."""
    family, cases, _ = G.GDN_TESTS[test]
    t_gemm, t_prod, rcp = G.GDN_FAMILIES[family]
    dtypes = (BF16,) if rcp == 'rcpf' else (F32,) if family == 'precise' else (BF16, F32)
    lines = []
    for case in cases:
        fam, x, w, t, params = G.gdn_case(test, kind, inverse, case)
        gamma, beta, label = params[2]
        assert fam == family and label == 'live gamma'
        n = E.gdn_norm(t, gamma, beta, t_gemm)                          # asserts: exact in f32, below 2^24 half quanta
        tb_exact = torch.equal(t.float().to(BF16).double(), t)
        if kind == 'narrow':
            assert tb_exact, 'narrow |t| must be bf16-exact'
        if family == 'precise':                                          # bf16x3 keeps two parts of |t|: they carry all of it
            a = t.abs().float()
            p0 = a.to(BF16).float()
            p1 = (a - p0).to(BF16).float()
            assert torch.equal(p0 + p1, a) and torch.equal((p0 + p1).double(), t.abs())
        want = {dt: E.gdn_restate(t, gamma, beta, inverse, t_gemm, t_prod, dt) for dt in dtypes}
        report = '{} {} {} inverse {}: max|t| {:.0f}'.format(test, case, kind, inverse, float(t.abs().max()))
        if not inverse:
            tp = t.float() if t_prod == F32 else t.float().to(BF16).float()
            nz = tp != 0
            y32 = E.gdn_restate(t, gamma, beta, False, t_gemm, t_prod, F32)
            share = float((y32 != tp / n)[nz].double().mean()) if bool(nz.any()) else 0.0
            report += ', t*(1/n) != t/n on {:.1%} of {} non-zero'.format(share, int(nz.sum()))
            assert share >= DISCRIMINATION_FLOOR, report          # (the two rcpf kernels store bf16 only: there it describes the operands)
            if rcp == 'rcpf':
                cands, many = E.gdn_admissible(t, gamma, beta, t_gemm, t_prod)
                amb = float(many.double().mean())
                report += ', ambiguous {:.4%}'.format(amb)
                if kind == 'narrow':
                    assert amb == 0.0, report
                    assert torch.equal(cands[0], (t / n.double()).to(BF16)), 'narrow: the one admissible value is cast(t / n)'
                else:
                    assert amb <= AMBIGUITY_CAP_WIDE, report
        # mutants of the restatement
        nzg = (gamma != 0).nonzero()
        o, c = (int(v) for v in nzg[len(nzg) // 2])
        g_drop = gamma.clone()
        g_drop[o, c] = 0
        C = gamma.shape[0]
        perm = list(range(C))
        perm[0], perm[1] = 1, 0
        gn = (n.double() - beta.double().view(1, -1, 1, 1)).float()      # gamma |t| alone
        tp = t.float() if t_prod == F32 else t.float().to(BF16).float()
        bb = beta.view(1, -1, 1, 1)
        late = tp * gn + bb if inverse else tp * (1.0 / gn + bb)         # beta joins behind the product / behind the reciprocal
        mutants = {
            'dropped gamma entry': lambda dt: E.gdn_restate(t, g_drop, beta, inverse, t_gemm, t_prod, dt),
            'gamma columns swapped': lambda dt: E.gdn_restate(t, gamma[:, perm], beta, inverse, t_gemm, t_prod, dt),
            'gamma rows swapped': lambda dt: E.gdn_restate(t, gamma[perm], beta, inverse, t_gemm, t_prod, dt),
            'beta late': lambda dt: late.to(dt),
        }
        for name, fn in mutants.items():
            changed = sum(_count(fn(dt), want[dt]) for dt in dtypes)
            report += ', {} {}'.format(name, changed)
            assert changed > 0, report
        for which in ('t_gemm', 't_prod'):
            flipped = {dt: E.gdn_restate(t, gamma, beta, inverse, _other(t_gemm) if which == 't_gemm' else t_gemm,
                                         _other(t_prod) if which == 't_prod' else t_prod, dt) for dt in dtypes}
            changed = sum(_count(flipped[dt], want[dt]) for dt in dtypes)
            report += ', {} flipped {}'.format(which, changed)
            if kind == 'narrow' or family == 'tile epilogue':      # bf16-exact t (the stand-alone GDN1's t IS a bf16 tensor): one precision only
                assert tb_exact and changed == 0, report
            elif which == 't_gemm':                                # every wide case of every fused family tells the precision of |t|
                assert not tb_exact and changed > 0, report
        if family == 'tile epilogue':       # the precise modes' launches of that test take the integers before their rounding to bf16
            pf = {p: E.gdn_restate(x, gamma, beta, inverse, p[0], p[1], F32) for p in ((F32, F32), (BF16, F32), (F32, BF16))}
            for p, name in (((BF16, F32), 't_gemm'), ((F32, BF16), 't_prod')):
                changed = _count(pf[p], pf[(F32, F32)])
                report += ', precise modes on the unrounded integers: {} flipped {}'.format(name, changed)
                assert changed == 0 if kind == 'narrow' else changed > 0, report
        lines.append(report)
    with capsys.disabled():
        print()
        for ln in lines:
            print('  ' + ln)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32, torch.int32])
@pytest.mark.parametrize('shape', [(3, 5, 7, 8), (1,), (130, 33)])
def test_arena_view_is_contiguous_aligned_and_surrounded_by_fill(dtype, shape):
    t = torch.arange(int(torch.tensor(shape).prod())).reshape(shape).to(dtype)
    v = E.arena(t)
    assert v.is_contiguous() and v.shape == t.shape and v.dtype == dtype and torch.equal(v, t)
    assert v.data_ptr() % E.ALIGN == 0
    raw, off, nbytes, value = v._arena
    assert off >= E.GUARD_BYTES and raw.numel() - off - nbytes >= E.GUARD_BYTES and nbytes == t.numel() * t.element_size()
    assert v.data_ptr() == raw.data_ptr() + off
    lo, hi, pattern = E.bands(v)
    assert lo.numel() * v.element_size() >= E.GUARD_BYTES and hi.numel() * v.element_size() >= E.GUARD_BYTES
    assert E.bands_untouched(v)
    band_lo = raw[:off].view(dtype)
    band_hi = raw[off + nbytes:].view(dtype)
    if dtype.is_floating_point:
        assert torch.isnan(band_lo).all() and torch.isnan(band_hi).all()
    else:
        assert (band_lo == E.INT_SENTINEL[dtype]).all() and (band_hi == E.INT_SENTINEL[dtype]).all()
    E.assert_bands_untouched(v, 'fresh')
    v.view(-1)[0] = 1          # writes inside the view leave the bands alone
    assert E.bands_untouched(v)
    raw[off + nbytes + 6:off + nbytes + 8] = 0      # one element past the end
    assert not E.bands_untouched(v)
    with pytest.raises(AssertionError) as e:
        E.assert_bands_untouched(v, 'past the end')
    assert 'ABOVE' in str(e.value)
    o = E.arena_like(shape, dtype, 'cpu')
    assert E.bands_untouched(o) and (torch.isnan(o).all() if dtype.is_floating_point else (o == E.INT_SENTINEL[dtype]).all())
