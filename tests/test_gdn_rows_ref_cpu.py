"""CPU: tests/ref_gdn_rows.py itself -- the float64 reference against autograd, the exactness conditions under which the GPU test
(tests/test_gpu_gdn_rows.py) may ask for equality, what its comparison function rejects, and the launch table for 256 compute
units.  Nothing here touches a kernel."""
import pytest
import torch

import ref_gdn_rows as R

P = 256
BF, F32, F64 = R.BF, R.F32, R.F64
_made = {}


def _case(C, M, kind):
    key = (C, M, kind)
    if key not in _made:
        if len(_made) > 6:
            _made.clear()
        _made[key] = R.make_case(C, M, kind, P)
    return _made[key]


# ---- the launch table, by hand, for P = 256 ----

@pytest.mark.parametrize('C,M,want', [
    (512, 1, (1, 1, 1, 1, None)), (512, 133, (2, 2, 1, 5, None)), (512, 128, (1, 1, 1, 128, None)),
    (512, 32768, (256, 256, 1, 128, None)), (512, 32769, (257, 256, 2, 1, 32768)),
    (256, 32769, (257, 256, 2, 1, 32768)), (256, 65903, (515, 256, 3, 111, 32768)), (256, 65536, (512, 256, 2, 128, 32768)),
    (96, 1, (1, 1, 1, 1, None)), (96, 33, (2, 1, 1, 1, None)), (96, 257, (9, 2, 1, 1, None)),
    (96, 65536, (2048, 256, 1, 32, None)), (96, 65537, (2049, 256, 2, 1, 65536)), (96, 131419, (4107, 256, 3, 27, 65536)),
])
def test_launch_table(C, M, want):
    L = R.launch(C, M, P)
    assert (L['units'], L['workgroups'], L['trips'], L['last_rows'], L['second_trip_row']) == want
    assert L['workers'] == L['workgroups'] * (8 if C == 96 else 1)


def test_case_table_for_256_cus():
    assert R.cases(P) == ((512, 1), (512, 133), (512, 32769), (256, 1), (256, 133), (256, 32769), (256, 65903),
                          (96, 1), (96, 33), (96, 65537), (96, 131419))
    assert set(R.small_cases()) <= set(R.cases(P)) and all(R.second_trip_case(C, P) in R.cases(P) for C in R.CHANNELS)
    assert max(M * C for C, M in R.cases(P)) * 2 < 34 << 20                        # the largest tensor: under 34 MB of bf16
    for cus in (64, 256, 304):                                                     # the tables reach the same paths on other devices
        trips = {(C, M): R.launch(C, M, cus)['trips'] for C, M in R.cases(cus)}
        assert sorted(set(trips.values())) == [1, 2, 3]
        for C in R.CHANNELS:
            L = R.launch(*R.second_trip_case(C, cus), cus)
            assert L['trips'] == 2 and L['last_rows'] == 1 and L['units'] == L['workers'] + 1


# ---- the reference against autograd ----

@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C,M', R.small_cases())
def test_reference_equals_autograd(C, M, kind):
    c = _case(C, M, kind)
    ref = R.reference_of(c)
    x = c['x'].to(F64).requires_grad_(True)
    gamma = c['gamma'].to(F64).requires_grad_(True)
    beta = c['beta'].to(F64).requires_grad_(True)
    n = beta + x.abs() @ gamma.t()                                                  # (autograd's abs: sign(0) = 0, the contract)
    y = x * n if c['inverse'] else x / n
    y.backward(c['g'].to(F64))
    assert torch.equal(y.detach(), ref['y'])
    for got, want in ((ref['dx'], x.grad), (ref['d_beta'], beta.grad), (ref['d_gamma'], gamma.grad)):
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)
    if kind != 'div':                                                              # integers and halves: autograd is exact too
        assert torch.equal(ref['dx'], x.grad) and torch.equal(ref['d_beta'], beta.grad) and torch.equal(ref['d_gamma'], gamma.grad)
    zero = c['x'] == 0
    assert torch.equal(ref['dx'][zero], ref['dd'][zero]) and bool((ref['dd'][zero] != 0).all())


# ---- the exactness conditions, every case and set ----

@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C,M', R.cases(P))
def test_exactness_conditions(C, M, kind):
    c = _case(C, M, kind)
    R.check_zeros(c, P)
    worst = R.check_exactness(c)
    print('C {} M {} {}: sum |terms| / quantum at most {}'.format(C, M, kind, {k: int(v) for k, v in worst.items()}))
    if kind == 'div':
        # every column of gamma is used, weights differ by column, rows by scale; the classes partition the channels
        g = c['gamma']
        assert bool((g != 0).any(0).all()) and len(torch.unique(c['w'])) == 3 and len(torch.unique(c['s'])) == 3
        assert torch.equal((g != 0), c['cls'][:, None] == c['cls'][None, :]) and torch.equal(c['beta'], c['s'])
        assert len(torch.unique(c['cls'])) == (4 if C == 96 else 8)
    else:
        assert set(torch.unique(c['gamma']).tolist()) <= {0.0, 0.5, 1.0, 2.0} and set(torch.unique(c['beta']).tolist()) <= {1.0, 2.0, 3.0}
        if kind == 'narrow':
            nzg = c['gamma'] != 0
            assert bool((nzg.sum(0) == 3).all()) and bool((nzg.sum(1) == 3).all())
    assert float(c['x'].abs().max()) <= 3 and float(c['g'].abs().max()) <= 3


def test_wide_set_exercises_the_rounding():
    """On 'wide' the bf16 store rounds (and meets ties); on 'narrow' and 'div' d_norm and the parked dd pass unrounded."""
    c = _case(256, 133, 'wide')
    ref = R.reference_of(c)
    for k in ('y', 'dx'):
        r = ref[k]
        rounded = R.cast(r, BF).to(F64) != r
        assert int(rounded.sum()) > r.numel() // 4, k
        ulp = 2.0 ** (torch.frexp(r.abs().clamp(min=1e-30))[1] - 8).to(F64)
        assert int(((r.abs() % ulp) == ulp / 2).sum()) > 100, k + ': no ties'


# ---- what the comparison rejects ----

def _rejects(mut64, ref64, dtype=BF):
    """the comparison of the GPU test, on a mutated reference rounded as a kernel would round it"""
    return int(R.differing(R.round_to(mut64, dtype), R.cast(ref64, dtype)).sum())


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C', R.CHANNELS)
def test_comparison_rejects_gamma_mutations(C, kind):
    """At M = 1, the smallest case: gamma transposed in either GEMM, one gamma term dropped, two gamma columns inside one 8-channel MFMA
    operand chunk swapped (the inverse sets)."""
    c = _case(C, 1, kind)
    ref = R.reference_of(c)
    x, gamma = c['x'], c['gamma']
    t1 = R.reference(x, c['g'], gamma.t().contiguous(), c['beta'], c['inverse'], gamma_bwd=gamma)
    assert _rejects(t1['y'], ref['y']) > 0, 'gamma^T in GEMM 1 passes'
    t2 = R.reference(x, c['g'], gamma, c['beta'], c['inverse'], gamma_bwd=gamma.t())
    assert torch.equal(t2['y'], ref['y']) and _rejects(t2['dx'], ref['dx']) > 0, 'gamma in place of gamma^T in GEMM 2 passes'
    # one term: gamma[i, j] with x[0, j] != 0 (GEMM 1), with dn[0, i] != 0 and x[0, j] != 0 (GEMM 2)
    live = (gamma != 0) & (x[0] != 0)[None, :] & (ref['d_norm'][0] != 0)[:, None]
    i, j = (int(v) for v in live.nonzero()[0])
    dropped = gamma.clone()
    dropped[i, j] = 0.0
    d1 = R.reference(x, c['g'], dropped, c['beta'], c['inverse'], gamma_bwd=gamma)
    bad = R.differing(R.round_to(d1['y'], BF), R.cast(ref['y'], BF))
    if kind != 'wide':                                                             # (wide: the store's rounding may hide half a quantum)
        assert bool(bad[0, i]) or float(x[0, i]) == 0.0, 'a dropped term of GEMM 1 passes'
        assert int(bad.sum()) <= 1
    d2 = R.reference(x, c['g'], gamma, c['beta'], c['inverse'], gamma_bwd=dropped)
    bad = R.differing(R.round_to(d2['dx'], BF), R.cast(ref['dx'], BF))
    if kind != 'wide':
        assert bool(bad[0, j]) and int(bad.sum()) == 1, 'a dropped term of GEMM 2 passes'
    else:                                                                          # wide: shown by some pixel of the next case
        cw = _case(C, 33 if C == 96 else 133, kind)
        rw = R.reference_of(cw)
        gw = cw['gamma']
        i, j = (int(v) for v in (gw == 2.0).nonzero()[0])
        less = gw.clone()
        less[i, j] = 0.0
        w1 = R.reference(cw['x'], cw['g'], less, cw['beta'], True, gamma_bwd=gw)
        w2 = R.reference(cw['x'], cw['g'], gw, cw['beta'], True, gamma_bwd=less)
        assert _rejects(w1['y'], rw['y']) > 0 and _rejects(w2['dx'], rw['dx']) > 0, 'a dropped term passes on the wide set'
    if kind != 'div':
        j1 = next(k for k in range(0, C, 8) if float(x[0, k].abs()) != float(x[0, k + 1].abs())
                  and not torch.equal(gamma[:, k], gamma[:, k + 1]))
        swapped = gamma.clone()
        swapped[:, [j1, j1 + 1]] = gamma[:, [j1 + 1, j1]]
        s1 = R.reference(x, c['g'], swapped, c['beta'], c['inverse'], gamma_bwd=gamma)
        s2 = R.reference(x, c['g'], gamma, c['beta'], c['inverse'], gamma_bwd=swapped)
        if kind == 'narrow':
            assert _rejects(s1['y'], ref['y']) + _rejects(s1['dx'], ref['dx']) > 0 and _rejects(s2['dx'], ref['dx']) > 0, 'swapped columns pass'
        else:
            assert _rejects(s1['dx'], ref['dx']) + _rejects(s2['dx'], ref['dx']) > 0, 'swapped columns pass'


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C', R.CHANNELS)
def test_comparison_rejects_zero_handling_mutations(C, kind):
    """At M = 1: the second term kept at one x == 0 element; one parked element lost."""
    c = _case(C, 1, kind)
    ref = R.reference_of(c)
    zero = (c['x'][0] == 0) & (ref['t'][0] != 0)
    if kind == 'wide':                                                             # (a t large enough to survive the store's rounding)
        zero &= ref['t'][0].abs() >= ref['dd'][0].abs() / 64
    j = int(zero.nonzero()[0])
    kept = ref['dx'].clone()
    kept[0, j] = ref['dd'][0, j] + ref['t'][0, j]
    assert _rejects(kept, ref['dx']) == 1, 'sign(0) = 1 passes'
    kept[0, j] = ref['dd'][0, j] - ref['t'][0, j]
    assert _rejects(kept, ref['dx']) == 1, 'sign(0) = -1 passes'
    lost = ref['dx'].clone()
    j = int((c['x'][0] == 0).nonzero()[-1])
    lost[0, j] = 0.0
    assert _rejects(lost, ref['dx']) == 1, 'a lost parked dd passes'
    lost[0, j] = ref['t'][0, j]
    assert _rejects(lost, ref['dx']) == 1, 'a lost parked dd passes'


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C', R.CHANNELS)
def test_comparison_rejects_a_d_beta_without_the_second_trip(C, kind):
    """At the smallest case with a second trip (its tile / strip holds one row): d_beta without that row."""
    C, M = R.second_trip_case(C, P)
    c = _case(C, M, kind)
    L = R.launch(C, M, P)
    assert L['second_trip_row'] == M - 1
    x, g = c['x'].to(F64), c['g'].to(F64)
    if c['inverse']:
        dn = g * x
    else:
        n = c['beta'].to(F64) + x.abs() @ c['gamma'].to(F64).t()
        dn = -g * x / (n * n)
    full, first_trip = dn.sum(0), dn[:L['second_trip_row']].sum(0)
    bad = R.differing(first_trip.to(F32), R.cast(full, F32))
    assert torch.equal(bad, dn[M - 1] != 0) and int(bad.sum()) >= 2


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C,M', [(512, 133), (256, 133), (96, 33)])
def test_comparison_rejects_an_unwritten_chunk_of_the_last_tile(C, M, kind):
    """One 16-byte chunk (8 channels) of the last row left as it was -- zeros, or the arena's sentinel."""
    c = _case(C, M, kind)
    ref = R.reference_of(c)
    for k in ('y', 'd_norm', 'dx'):
        want = R.cast(ref[k], BF)
        row = want[M - 1].view(C // 8, 8)
        chunk = int((row != 0).any(1).nonzero()[-1])
        for fill in (0.0, torch.tensor([0x5A5A], dtype=torch.int16).view(BF).item()):
            got = want.clone()
            got[M - 1, chunk * 8:chunk * 8 + 8] = fill
            n = int(R.differing(got, want).sum())
            assert 1 <= n <= 8, k
            with pytest.raises(AssertionError, match='pixel: 1 distinct, {}'.format(M - 1)):
                R.assert_same(got, want, k, R.UNIT_ROWS[C])
        assert R.assert_same(want.clone(), want, k) == 0
    nan = R.cast(ref['y'], BF).clone()
    nan[0, 0] = float('nan')
    assert int(R.differing(nan, nan).sum()) == 1                                   # (a NaN never passes, whatever the reference holds)
