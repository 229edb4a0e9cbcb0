"""-m gpu: sc2_bn_train_fwd / sc2_bn_train_bwd (csrc/bn.hip) against the float64 reference of tests/ref_bn.py, called directly through
hip.bn_train_fwd / hip.bn_train_bwd (and, for the arena test, through the C entry points), element by element.

test_bn_train_kernels (tests/test_gpu_kernels.py) compares y and dx by relative L2 norm over the whole tensor (< 3e-3) at power-of-two
widths: bf16 rounding alone gives 1e-3 there, and a wrong last row, one wrong 8-channel chunk or a mask taken from the neighbouring
element disappear under it.  Here:

  bf16 outputs (y, dx)   every element: |got - ref| <= 2^-8 |ref| + slack * scale -- the single bf16 rounding the kernel is allowed plus
                         the f32 arithmetic in front of it; dz is a pure select (dy or 0) and is compared bit for bit.
  f32 per-channel        every channel: |got - ref| <= slack * scale_c; scale = rms(x_c) for save_mean, rstd_c for save_rstd, sum |dz|
                         for dbeta, sum |dz xhat| for dgamma, the new value's magnitude plus the update's scale for the running
                         statistics (ref_bn.scales_fwd / scales_bwd; element scales for y and dx: the magnitudes of the terms summed).
  slack                  F32_MARGIN = 8 times the error of the float32 form of the SAME reference under the same metric
                         (ref_bn.E_F32_MAX, measured and re-measured by tests/test_bn_ref_cpu.py) -- never anything measured on the
                         kernel.  The device sums in another order, contracts a * b + c and its sqrt / division may differ by an ulp;
                         nothing else separates the two.
  cases                  ref_bn.CASES, M rows of C channels (cpr = C / 8, ppi = 512 // cpr, nb = clamp(ceil(M / (8 ppi)), 1, 512)):

      C     M      cpr / ppi / idle   nb   reaches
      8     2      1 / 512 / 0        1    smallest legal M (unbiased factor 2); 510 threads own no row; finalize workgroup 8 of 32 live
      24    1361   3 / 170 / 2        2    idle threads; exactly one row (1360) past the last full trip: the `live` select, the clamped load
      128   2049   16 / 32 / 0        9    slice 0 adds two partial rows, the other slices one
      40    19585  5 / 102 / 2        25   smallest nb at which slice 0 enters the unrolled loop of bn_sum_partials; slices 1..7 tail only
      72    14337  9 / 56 / 8         33   unrolled loop THEN tail in slice 0
      1032  100    129 / 3 / 125      5    almost two waves idle; last finalize workgroup 8 of 32 live
      2040  37     255 / 2 / 2        3    widest non-power-of-two cpr; last finalize workgroup 24 live
      2048  8200   256 / 2 / 0        512  nb at its cap with ragged trips; 2 099 200 chunks: a second grid-stride trip of both stream kernels

                         sc2_bn_ws_floats(M, C) must equal nb * 2 C + 3 C of the restated arithmetic (ref_bn.launch), so each case
                         really reaches its nb.  Every case runs both directions with relu x residual in all four combinations, dz
                         asked for and not, y = NULL in the backward of the no-ReLU combinations, each launch twice (bit-equal: no
                         atomics).  C = 24 also runs momentum 0.25 / eps 1e-3.
  backward operands      y = the float64 forward rounded to bf16, save_mean / save_rstd = the float64 statistics rounded to f32: the
                         backward is tested independently of the device forward, and the mask is decidable everywhere.
Also: running statistics absent (bit-identical y and saved statistics), the refusals, sentinel arenas around every output and the
scratch, and NaN propagation through the ReLU (one NaN in x: its channel is NaN, never zeros; every other channel meets its bound).
Measured on an MI355X (profiles/r20_gpu_bn_train.log), largest over all cases, next to the bound: y 3.4e-7 (8.9e-6),
dx 2.8e-8 (6.1e-6), save_mean 1.4e-7 (1.2e-6), save_rstd 2.0e-6 (8.6e-6), running_mean 1.2e-7 (1.1e-6), running_var 2.1e-7 (9.5e-7), dbeta
2.5e-8 (2.0e-7), dgamma 1.5e-7 (4.7e-6).  The NaN test failed on the kernel as it was (a channel of zeros; a finite save_rstd and
running_var from the variance clamp): both were faults of the kernel and are fixed there.
"""
import pytest
import torch

import ref_bn as B

pytestmark = pytest.mark.gpu

BOUND = {k: B.F32_MARGIN * v for k, v in B.E_F32_MAX.items()}
_cases = {}


def _case(C, M, dev):
    """The case's operands on the device: f32 as generated, '<name>_bf16' for the kernels' bf16 operands as [1, M, 1, C]."""
    if (C, M) not in _cases:
        c = B.make_case(C, M)
        d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
        for k in ('x', 'residual', 'dy'):
            d[k + '_bf16'] = d[k].to(torch.bfloat16).view(1, M, 1, C).contiguous()
            assert torch.equal(d[k + '_bf16'].float().view(M, C), d[k])
        if M * C > 1 << 22:                       # (the largest case runs once: not kept on the device)
            return d
        _cases[C, M] = d
    return _cases[C, M]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _report(tag, errors, failures):
    print(tag + ': ' + '  '.join('{} {:.2e} ({:.2e})'.format(k, e, BOUND[k]) for k, e in errors.items()))
    failures.extend((tag, k, e, BOUND[k]) for k, e in errors.items() if not e <= BOUND[k])


def _run_both(S, d, ref, relu, res, momentum, eps, cols=None):
    """One forward and one backward on case d, both launched twice -> the errors under ref_bn's metrics (over the channels `cols`,
    all by default) and the raw outputs."""
    hip = S.hip
    M, C = d['M'], d['C']
    cols = slice(None) if cols is None else cols
    residual = d['residual'] if res else None
    f = ref.forward(relu, residual)
    out = []
    for _ in range(2):
        rm, rv = d['running_mean'].clone(), d['running_var'].clone()
        y, mean, rstd = hip.bn_train_fwd(d['x_bf16'], d['gamma'], d['beta'], rm, rv, momentum, eps, relu,
                                         residual=d['residual_bf16'] if res else None)
        out.append((y, mean, rstd, rm, rv))
    assert _same(*out), 'two forward launches on equal inputs differ'
    assert y.dtype == torch.bfloat16 and y.shape == (1, M, 1, C) and mean.shape == rstd.shape == (C,)
    sc = B.scales_fwd(ref, residual, momentum)
    errors = {'y': B.err_bf16(y.view(M, C)[:, cols], f['y'][:, cols], sc['y'][:, cols]),
              'save_mean': B.err(mean[cols], f['mean'][cols], sc['save_mean'][cols]),
              'save_rstd': B.err(rstd[cols], f['rstd'][cols], sc['save_rstd'][cols]),
              'running_mean': B.err(rm[cols], f['running_mean'][cols], sc['running_mean'][cols]),
              'running_var': B.err(rv[cols], f['running_var'][cols], sc['running_var'][cols])}
    # the backward on the REFERENCE's y and statistics
    y_ref = f['y'].to(torch.bfloat16).view(1, M, 1, C).contiguous() if relu else None
    b = ref.backward(d['dy'], None if y_ref is None else y_ref.view(M, C))
    args = (d['dy_bf16'], d['x_bf16'], y_ref, d['gamma'], f['mean'].float(), f['rstd'].float())
    dx, dz, dg, db = hip.bn_train_bwd(*args, want_dz=True)
    assert _same((dx, dz, dg, db), hip.bn_train_bwd(*args, want_dz=True)), 'two backward launches on equal inputs differ'
    dx2, none, dg2, db2 = hip.bn_train_bwd(*args, want_dz=False)
    assert none is None and _same((dx, dg, db), (dx2, dg2, db2)), 'the backward without dz differs'
    want_dz = d['dy_bf16'] if y_ref is None else torch.where(y_ref > 0, d['dy_bf16'], torch.zeros_like(d['dy_bf16']))
    dz_exact = torch.equal(_bits(dz).view(M, C)[:, cols], _bits(want_dz).view(M, C)[:, cols])
    sb = B.scales_bwd(ref, b)
    errors.update({'dx': B.err_bf16(dx.view(M, C)[:, cols], b['dx'][:, cols], sb['dx'][:, cols]),
                   'dbeta': B.err(db[cols], b['dbeta'][cols], sb['dbeta'][cols]),
                   'dgamma': B.err(dg[cols], b['dgamma'][cols], sb['dgamma'][cols])})
    return errors, dz_exact, dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, dx=dx, dz=dz, dg=dg, db=db)


def test_workspace_is_the_restated_launch_arithmetic(S, dev):
    lib = S.hip.lib()
    for C, M, cpr, ppi, idle, nb in B.CASES:
        L = B.launch(M, C)
        assert (L['cpr'], L['ppi'], L['idle'], L['nb']) == (cpr, ppi, idle, nb)
        assert lib.sc2_bn_ws_floats(M, C) == L['ws_floats'] == nb * 2 * C + 3 * C, (C, M)
    for M, C in ((19584, 40), (14336, 72), (8192, 2048), (1360, 24), (1, 8), (10 ** 9, 8)):     # the thresholds from the other side
        assert lib.sc2_bn_ws_floats(M, C) == B.launch(M, C)['ws_floats'], (M, C)
    assert lib.sc2_bn_ws_floats(5, 12) == 0 and lib.sc2_bn_ws_floats(5, 2056) == 0 and lib.sc2_bn_ws_floats(0, 8) == 0


@pytest.mark.parametrize('C,M,momentum,eps', B.variants(), ids=['{}x{}-m{}'.format(C, M, m) for C, M, m, _ in B.variants()])
def test_bn_kernels_element_by_element(S, dev, C, M, momentum, eps):
    d = _case(C, M, dev)
    assert S.hip.lib().sc2_bn_ws_floats(M, C) == B.launch(M, C)['ws_floats']
    ref = B.BnRef(d['x'], d['gamma'], d['beta'], d['running_mean'], d['running_var'], momentum, eps)
    assert float(ref.mean[2]) == 0.5 and float(ref.var[2]) == 0.0                # the constant channel is exact in the reference here too
    failures = []
    for relu, res in B.COMBOS:
        tag = 'bn {}x{} momentum {} eps {} relu {:d} residual {:d}'.format(C, M, momentum, eps, relu, res)
        errors, dz_exact, _ = _run_both(S, d, ref, relu, res, momentum, eps)
        _report(tag, errors, failures)
        if not dz_exact:
            failures.append((tag, 'dz is not the select of dy'))
    assert not failures, failures


def test_running_statistics_absent(S, dev):
    C, M = 24, 1361
    d = _case(C, M, dev)
    for relu, res in B.COMBOS:
        r = d['residual_bf16'] if res else None
        rm, rv = d['running_mean'].clone(), d['running_var'].clone()
        with_stats = S.hip.bn_train_fwd(d['x_bf16'], d['gamma'], d['beta'], rm, rv, 0.1, 1e-5, relu, residual=r)
        without = S.hip.bn_train_fwd(d['x_bf16'], d['gamma'], d['beta'], None, None, 0.1, 1e-5, relu, residual=r)
        assert _same(with_stats, without)
        assert not torch.equal(rm, d['running_mean']) and not torch.equal(rv, d['running_var'])
    lib, hip = S.hip.lib(), S.hip                                                                 # one without the other is refused
    y, st, rm = torch.full_like(d['x_bf16'], 3.0), torch.empty(2, C, device=dev), d['running_mean'].clone()
    ws = torch.empty(int(lib.sc2_bn_ws_floats(M, C)), device=dev)
    for a, b in ((hip._ptr(rm), None), (None, hip._ptr(rm))):
        rc = lib.sc2_bn_train_fwd(hip._ptr(d['x_bf16']), None, hip._ptr(d['gamma']), hip._ptr(d['beta']), a, b, 0.1, 1e-5, 1, hip._ptr(y),
                                  st[0].data_ptr(), st[1].data_ptr(), hip._ptr(ws), M, C, hip._stream())
        assert rc == -1 and bool((y == 3.0).all()) and torch.equal(rm, d['running_mean'])


def test_refusals(S, dev):
    hip, lib = S.hip, S.hip.lib()

    def operands(M, C):
        x = torch.zeros(1, M, 1, C, dtype=torch.bfloat16, device=dev)
        v = torch.ones(C, device=dev)
        return x, v
    x, v = operands(1, 8)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        hip.bn_train_fwd(x, v, v, v.clone(), v.clone(), 0.1, 1e-5, True)
    y, ws, o1, o2 = torch.full_like(x, 3.0), torch.empty(64, device=dev), v.clone(), v.clone()
    rc = lib.sc2_bn_train_fwd(hip._ptr(x), None, hip._ptr(v), hip._ptr(v), None, None, 0.1, 1e-5, 1, hip._ptr(y), hip._ptr(o1),
                              hip._ptr(o2), hip._ptr(ws), 1, 8, hip._stream())
    assert rc == -1 and bool((y == 3.0).all())                                                    # refused, nothing launched
    for C in (12, 2056):
        x, v = operands(4, C)
        with pytest.raises(ValueError):
            hip.bn_train_fwd(x, v, v, v.clone(), v.clone(), 0.1, 1e-5, True)
        with pytest.raises(ValueError):
            hip.bn_train_bwd(x, x, None, v, v, v)
        y, dx, ws, o1, o2 = torch.full_like(x, 3.0), torch.full_like(x, 3.0), torch.empty(8 * C, device=dev), v.clone(), v.clone()
        rc = lib.sc2_bn_train_fwd(hip._ptr(x), None, hip._ptr(v), hip._ptr(v), None, None, 0.1, 1e-5, 1, hip._ptr(y),
                                  hip._ptr(o1), hip._ptr(o2), hip._ptr(ws), 4, C, hip._stream())
        assert rc == -1 and bool((y == 3.0).all())
        rc = lib.sc2_bn_train_bwd(hip._ptr(x), hip._ptr(x), None, hip._ptr(v), hip._ptr(v), hip._ptr(v), hip._ptr(dx), None,
                                  hip._ptr(o1), hip._ptr(o2), hip._ptr(ws), 4, C, hip._stream())
        assert rc == -1 and bool((dx == 3.0).all())


class _Arena(object):
    """`n` elements of bf16 (as int16) or f32 (as int32) between two bands of PAD sentinel elements."""
    PAD = 4096                              # (elements: the payload stays 16-byte aligned)

    def __init__(self, n, dtype, dev, init=None):
        self.int_dtype, self.sentinel = (torch.int16, 0x5A5A) if dtype == torch.bfloat16 else (torch.int32, 0x5A5A5A5A)
        self.n, self.dtype = n, dtype
        self.buf = torch.full((n + 2 * self.PAD,), self.sentinel, dtype=self.int_dtype, device=dev)
        if init is not None:
            self.payload().copy_(init.reshape(-1))
        assert self.ptr() % 16 == 0

    def payload(self):
        return self.buf[self.PAD:self.PAD + self.n].view(self.dtype)

    def ptr(self):
        return self.buf.data_ptr() + self.PAD * self.buf.element_size()

    def bands_untouched(self):
        return bool((self.buf[:self.PAD] == self.sentinel).all()) and bool((self.buf[self.PAD + self.n:] == self.sentinel).all())

    def fully_written(self):
        return not bool((self.buf[self.PAD:self.PAD + self.n] == self.sentinel).any())


@pytest.mark.parametrize('C,M', [(24, 1361), (1032, 100)])
def test_outputs_and_scratch_stay_inside_their_extents(S, dev, C, M):
    """The C entry points with y, dx, dz, the six per-channel vectors and ws (exactly sc2_bn_ws_floats floats) inside sentinel-filled
    arenas: every byte outside the declared extents is unchanged, every output element is written, and the results are the wrapper's."""
    hip, lib = S.hip, S.hip.lib()
    d = _case(C, M, dev)
    n_ws = int(lib.sc2_bn_ws_floats(M, C))
    assert n_ws == B.launch(M, C)['ws_floats']
    bf, f32 = torch.bfloat16, torch.float32
    a = dict(y=_Arena(M * C, bf, dev), dx=_Arena(M * C, bf, dev), dz=_Arena(M * C, bf, dev), save_mean=_Arena(C, f32, dev),
             save_rstd=_Arena(C, f32, dev), running_mean=_Arena(C, f32, dev, d['running_mean']),
             running_var=_Arena(C, f32, dev, d['running_var']), dgamma=_Arena(C, f32, dev), dbeta=_Arena(C, f32, dev),
             ws_fwd=_Arena(n_ws, f32, dev), ws_bwd=_Arena(n_ws, f32, dev))
    rc = lib.sc2_bn_train_fwd(hip._ptr(d['x_bf16']), hip._ptr(d['residual_bf16']), hip._ptr(d['gamma']), hip._ptr(d['beta']),
                              a['running_mean'].ptr(), a['running_var'].ptr(), 0.1, 1e-5, 1, a['y'].ptr(), a['save_mean'].ptr(),
                              a['save_rstd'].ptr(), a['ws_fwd'].ptr(), M, C, hip._stream())
    assert rc == 0
    y = a['y'].payload().view(1, M, 1, C)
    rc = lib.sc2_bn_train_bwd(hip._ptr(d['dy_bf16']), hip._ptr(d['x_bf16']), y.data_ptr(), hip._ptr(d['gamma']), a['save_mean'].ptr(),
                              a['save_rstd'].ptr(), a['dx'].ptr(), a['dz'].ptr(), a['dgamma'].ptr(), a['dbeta'].ptr(), a['ws_bwd'].ptr(),
                              M, C, hip._stream())
    assert rc == 0
    torch.cuda.synchronize()
    for name, arena in a.items():
        assert arena.bands_untouched(), 'a write outside ' + name
        if not name.startswith('ws'):
            assert arena.fully_written(), 'an element of {} was left unwritten'.format(name)
    # the partial sums and the backward's three coefficient rows are all written; the forward uses two of the three rows
    assert a['ws_bwd'].fully_written()
    assert not bool((a['ws_fwd'].buf[a['ws_fwd'].PAD:a['ws_fwd'].PAD + n_ws - C] == a['ws_fwd'].sentinel).any())
    rm, rv = d['running_mean'].clone(), d['running_var'].clone()
    y2, mean2, rstd2 = hip.bn_train_fwd(d['x_bf16'], d['gamma'], d['beta'], rm, rv, 0.1, 1e-5, True, residual=d['residual_bf16'])
    dx2, dz2, dg2, db2 = hip.bn_train_bwd(d['dy_bf16'], d['x_bf16'], y2, d['gamma'], mean2, rstd2, want_dz=True)
    got = [a[k].payload() for k in ('y', 'save_mean', 'save_rstd', 'running_mean', 'running_var', 'dx', 'dz', 'dgamma', 'dbeta')]
    assert _same(got, [t.reshape(-1) for t in (y2, mean2, rstd2, rm, rv, dx2, dz2, dg2, db2)])


@pytest.mark.parametrize('res', [False, True], ids=['plain', 'residual'])
def test_nan_propagates_through_the_relu(S, dev, res):
    """One NaN in channel 3 of x, relu=True: torch returns a NaN channel (mean and variance are NaN, torch.relu propagates NaN), and so
    must this kernel -- a channel of zeros would let a diverged run go on with finite activations.  Channel 3 of y, save_mean, save_rstd,
    running_mean, running_var and dx is NaN throughout; every other channel meets its ordinary bound.  (Left unspecified: the gradient
    torch would pass through a NaN output -- dz and dbeta of that channel; the sign of a zero.)"""
    C, M, ch = 24, 1361, B.NAN_CHANNEL
    d = dict(_case(C, M, dev))
    d['x'] = d['x'].clone()
    d['x'][700, ch] = float('nan')
    d['x_bf16'] = d['x'].to(torch.bfloat16).view(1, M, 1, C).contiguous()
    ref = B.BnRef(d['x'], d['gamma'], d['beta'], d['running_mean'], d['running_var'])
    f = ref.forward(True, d['residual'] if res else None)
    assert bool(torch.isnan(f['y'][:, ch]).all()) and int(torch.isnan(f['y']).sum()) == M        # what torch's semantics give
    others = [c for c in range(C) if c != ch]
    errors, dz_exact, out = _run_both(S, d, ref, True, res, 0.1, 1e-5, cols=others)
    failures = []
    _report('bn 24x1361 NaN in channel 3, residual {:d}'.format(res), errors, failures)
    assert not failures and dz_exact, failures
    y, dx = out['y'].view(M, C), out['dx'].view(M, C)
    assert bool(torch.isnan(y[:, ch]).all()), 'channel 3 of y: {} NaN, {} zeros of {}'.format(
        int(torch.isnan(y[:, ch]).sum()), int((y[:, ch] == 0).sum()), M)
    for name in ('mean', 'rstd', 'rm', 'rv'):
        assert bool(torch.isnan(out[name][ch])), name
    assert bool(torch.isnan(dx[:, ch]).all())
    assert int(torch.isnan(y).sum()) == M and int(torch.isnan(dx).sum()) == M                     # and nowhere else
