"""Float64 reference, dyadic operand builders and case tables for the resident-row GDN1 kernels (csrc/gdn512_rows.hip: C = 512 / 256,
csrc/gdn96_strips.hip: C = 96): test infrastructure only, imported by tests/test_gdn_rows_ref_cpu.py and tests/test_gpu_gdn_rows.py.

The operation, on [M, C] operands, as the two kernel headers state it:

  n = beta + |x| gamma^T
  forward    y = x * n  (inverse)                    |  x / n
  backward   dd = g * n, dn = g * x  (inverse)       |  dd = g / n, dn = -dd * x / n
             dx = dd + sign(x) * (dn gamma), sign(0) = 0;  d_norm = dn;  d_beta = colsum(dn);  d_gamma = dn^T |x|

Operand sets (`KINDS`).  All are dyadic: every f32 intermediate of the kernels is exact in any order of summation, with or without FMA
contraction, through the bf16 image of dn that feeds GEMM 2 and through the d_beta atomics (tests/test_gdn_rows_ref_cpu.py proves the
conditions on this reference for every case).  A correct kernel therefore EQUALS `cast(reference)`: one rounding to bf16 of an
exact f32 value, d_beta the f32 value itself.  No tolerance.  (Compared as values: the sign of a zero is left open -- the kernels
form dx as sign(x) * (sign(x) dd + t), which gives -0 where the reference's dd + sign(x) t gives +0 -- and nothing may be non-finite.)

  narrow  inverse form, integer-closed: x, g in {-3..3}, beta in {1, 2, 3}, gamma with exactly three entries of {1/2, 1, 2} in
          every row and every column (three random diagonals): n <= 3 + 3 * 6 = 21, |y| <= 63, |dx| <= 63 + 3 * 18 = 117, |d_norm| <= 9,
          all multiples of 1/2 -- at most 256 quanta (asserted by `check_exactness`), so every output is bf16-exact and ONE missing or
          misplaced term shows through the bf16 store; the parked dd is bf16-exact too.
  wide    the same with gamma uniform in {0, 1/2, 1, 2}: outputs run into the thousands, the bf16 store's rounding and its ties are
          exercised.  (Here a parked dd is exact in f32 but not in bf16: the kernel rounds it once when it parks it, the reference
          once in `cast` -- the same rounding of the same number.  The two-launch form of hip.gdn1_backward rounds dd to bf16 BETWEEN
          its launches and adds to the rounded value, so the composition test runs on 'narrow' and 'div', where dd is bf16-exact.)
  div     forward (division) form with every norm a power of two, so that 1.0f / n and all three products are exact.  The channels
          fall into r classes of equal size (a random permutation dealt round-robin; r = 4 at C = 96, else 8); gamma[i, j] =
          s_i * w_j for class(i) == class(j), else 0, with s_i in {1/2, 1, 2}, w_j in {1, 2, 3} and the first four columns of every class
          reserved with w = 1; beta_i = s_i, so n_i = s_i * (1 + sum_j w_j |x_j|) over the class of i.  Per pixel and class up to two
          free columns draw |x| in {0..3} (a draw that would take the weighted sum past 15 is dropped), then the reserved columns
          are set so that 1 + sum_j w_j |x_j| is the next of {2, 4, 8, 16}.  Every column of gamma is used, weights differ by column,
          rows by scale.  The all-zero pixel (and the rows a tile holds past the end of the tensor) have n_i = s_i: a power of two too.
          g in {-3..3}.  If a device's 1.0f / 2^k were not exact every element would fail at once: to be reported, not loosened.

Zeros of x, in every case (`zero_plan`): a whole pixel (row 1; left out where M < 3, so that a one- or two-pixel case still runs its
GEMMs on live data), a whole channel, about 1 % single elements, one -0, a +0 and the -0 in the last valid row, and where the case
has a second trip two zeros in a row of a second-trip tile / strip.  g != 0 at every zero of x and in the whole last row: a lost
parked dd, or a d_beta that misses the last row, is a gross error.

`launch(C, M, cus)` restates the launchers' arithmetic; the GPU test holds it against what the library reports
(sc2_gdn1_rows_units, sc2_gdn1_rows_workgroups).  `cases(P)` are functions of the device's CU count P."""
import torch

import exact_ints as E

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
KINDS = ('narrow', 'wide', 'div')
CHANNELS = (512, 256, 96)
UNIT_ROWS = {512: 128, 256: 128, 96: 32}       # pixels of a tile (one workgroup) / of a strip (one wave)
STRIP_WAVES = 8
LIMIT_BYTES = 0x7FF00000
RESERVED = 4                                   # div: columns per class that make the norm a power of two
EXACT_LIMIT = E.EXACT_LIMIT
NARROW_QUANTA = E.NARROW_MAX


# --------------------------------------------------------------------------------------------- #
# launch arithmetic, cases
# --------------------------------------------------------------------------------------------- #
def launch(C, M, cus):
    """units: tiles (C = 256 / 512) or strips (C = 96); workgroups; workers: the units taken per trip (a workgroup owns a tile, a wave a
    strip); trips of the busiest worker; last_rows: rows live in the last unit; second_trip_row: first row of the first unit that
    is some worker's second, or None."""
    assert C in UNIT_ROWS and M > 0 and M * C * 2 < LIMIT_BYTES
    rows = UNIT_ROWS[C]
    units = (M + rows - 1) // rows
    if C == 96:
        workgroups = min((units + STRIP_WAVES - 1) // STRIP_WAVES, cus)
        workers = workgroups * STRIP_WAVES
    else:
        workgroups = workers = min(units, cus)
    trips = (units + workers - 1) // workers
    return dict(units=units, workgroups=workgroups, workers=workers, trips=trips, last_rows=M - (units - 1) * rows,
                second_trip_row=workers * rows if trips > 1 else None)


CASE_NAMES = ('one', 'two_units', 'second_trip', 'third_trip')
CASE_IDS = tuple((C, name) for C in CHANNELS for name in CASE_NAMES if not (C == 512 and name == 'third_trip'))   # (512: to bound memory)
SMALL_IDS = tuple((C, name) for C in CHANNELS for name in CASE_NAMES[:2])


def case_rows(C, name, P):
    """M of a named case on a device of P compute units: 'one' pixel; 'two_units': a partial second tile on a second workgroup / a
    second wave with one row; 'second_trip': exactly one worker takes a second unit, holding one row; 'third_trip': third trips and a
    ragged last unit."""
    if C == 96:
        return {'one': 1, 'two_units': 33, 'second_trip': 32 * 8 * P + 1, 'third_trip': 32 * (16 * P + 11) - 5}[name]
    return {'one': 1, 'two_units': 133, 'second_trip': 128 * P + 1, 'third_trip': 128 * (2 * P + 3) - 17}[name]


def small_cases():
    return tuple((C, case_rows(C, name, 1)) for C, name in SMALL_IDS)


def cases(P):
    """(C, M) for a device of P compute units."""
    return tuple((C, case_rows(C, name, P)) for C, name in CASE_IDS)


def second_trip_case(C, P):
    return (C, case_rows(C, 'second_trip', P))


# --------------------------------------------------------------------------------------------- #
# operands
# --------------------------------------------------------------------------------------------- #
def zero_plan(C, M, cus, cols):
    """Where x is forced to zero; cols: the channels that may be zeroed (div: the free columns), in a fixed order."""
    L = launch(C, M, cus)
    pick = lambda k: int(cols[k % len(cols)])
    plan = dict(pixel=1 if M >= 3 else None, channel=pick(37), last=(M - 1, pick(5)), neg_zero=(M - 1, pick(9)), second=None)
    if L['second_trip_row'] is not None:
        row = min(L['second_trip_row'] + 3, M - 1)
        plan['second'] = ((row, pick(14)), (row, pick(21)))
    return plan


def _apply_zeros(x, plan, cols, g):
    """Zeros onto x (values or magnitudes): the plan's, and about 1 % single elements of `cols`."""
    M = x.shape[0]
    single = torch.zeros(x.shape, dtype=torch.bool)
    single[:, cols] = torch.rand((M, len(cols)), generator=g) < 0.01
    x[single] = 0.0
    x[:, plan['channel']] = 0.0
    for pos in (plan['last'], plan['neg_zero']) + (plan['second'] or ()):
        x[pos] = 0.0
    return x


def _gradient(x, M, C, g):
    gy = torch.randint(-3, 4, (M, C), generator=g).float()
    gy[(x == 0) & (gy == 0)] = 1.0
    last = gy[M - 1]
    last[last == 0] = -2.0
    return gy


def make_case(C, M, kind, cus=256):
    """-> dict: x, g [M, C], gamma [C, C], beta [C] as f32 on the CPU (all exact in bf16), inverse, plan (zero_plan)."""
    assert kind in KINDS
    g = E.gen(C, M, KINDS.index(kind), 20261)
    if kind == 'div':
        return _make_div(C, M, cus, g)
    cols = torch.arange(C)
    plan = zero_plan(C, M, cus, cols)
    vals = torch.tensor([0.5, 1.0, 2.0])
    if kind == 'narrow':
        gamma = torch.zeros(C, C)
        offs = torch.randperm(C, generator=g)[:3]
        i = torch.arange(C)
        for o in offs:
            gamma[i, (i + int(o)) % C] = vals[torch.randint(0, 3, (C,), generator=g)]
    else:
        gamma = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (C, C), generator=g)]
    beta = torch.randint(1, 4, (C,), generator=g).float()
    x = _apply_zeros(torch.randint(-3, 4, (M, C), generator=g).float(), plan, cols, g)
    if plan['pixel'] is not None:
        x[plan['pixel']] = 0.0
    x[plan['neg_zero']] = -0.0
    return dict(x=x, g=_gradient(x, M, C, g), gamma=gamma, beta=beta, inverse=True, plan=plan, kind=kind)


def _make_div(C, M, cus, g):
    r = 4 if C == 96 else 8
    nc = C // r
    members = torch.randperm(C, generator=g).view(nc, r).t().contiguous()          # [r, nc]: the channels of class k, reserved ones first
    cls = torch.empty(C, dtype=torch.long)
    cls[members.reshape(-1)] = torch.arange(r).repeat_interleave(nc)
    w_local = torch.randint(1, 4, (r, nc), generator=g).float()
    w_local[:, :RESERVED] = 1.0
    w = torch.empty(C)
    w[members.reshape(-1)] = w_local.reshape(-1)
    s = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    gamma = s[:, None] * w[None, :] * (cls[:, None] == cls[None, :]).float()
    free = members[:, RESERVED:].reshape(-1).sort().values
    plan = zero_plan(C, M, cus, free)
    # up to two free columns per pixel and class
    a = torch.randint(RESERVED, nc, (M, r), generator=g)
    b = torch.randint(RESERVED, nc, (M, r), generator=g)
    va = torch.randint(0, 4, (M, r), generator=g).float()
    vb = torch.randint(0, 4, (M, r), generator=g).float()
    k = torch.arange(r)[None, :].expand(M, r)
    vb[(b == a) | (va * w_local[k, a] + vb * w_local[k, b] > 15)] = 0.0
    xl = torch.zeros(M, r, nc)
    xl.scatter_(2, a[..., None], va[..., None])
    xl.scatter_add_(2, b[..., None], vb[..., None])
    ax = torch.zeros(M, C)
    ax[:, members.reshape(-1)] = xl.reshape(M, C)
    ax = _apply_zeros(ax, plan, free, g)
    # the reserved columns: 1 + sum_j w_j |x_j| becomes the next of {2, 4, 8, 16}
    xl = ax[:, members.reshape(-1)].reshape(M, r, nc)
    S = (xl[..., RESERVED:] * w_local[:, RESERVED:]).sum(-1)
    assert float(S.max()) <= 15
    T = torch.where(S <= 1, 2.0, torch.where(S <= 3, 4.0, torch.where(S <= 7, 8.0, 16.0)))
    d = T - 1 - S
    for q in range(RESERVED):
        v = d.clamp(max=3.0)
        xl[..., q] = v
        d = d - v
    assert float(d.abs().max()) == 0
    ax[:, members.reshape(-1)] = xl.reshape(M, C)
    if plan['pixel'] is not None:
        ax[plan['pixel']] = 0.0
    sign = torch.randint(0, 2, (M, C), generator=g).float() * 2 - 1
    x = sign * ax + 0.0                                                            # (+ 0.0: no -0 but the one placed below)
    x[plan['neg_zero']] = -0.0
    return dict(x=x, g=_gradient(x, M, C, g), gamma=gamma, beta=s.clone(), inverse=False, plan=plan, kind='div', cls=cls, members=members,
                s=s, w=w)


# --------------------------------------------------------------------------------------------- #
# reference
# --------------------------------------------------------------------------------------------- #
def sign(x):
    return (x > 0).to(x.dtype) - (x < 0).to(x.dtype)


def reference(x, g, gamma, beta, inverse, gamma_bwd=None):
    """Float64, on the operands' device.  gamma_bwd: the matrix whose TRANSPOSE multiplies dn (default gamma; a mutation hook)."""
    x, g, gamma, beta = (t.to(F64) for t in (x, g, gamma, beta))
    gb = gamma if gamma_bwd is None else gamma_bwd.to(F64)
    ax = x.abs()
    n = beta + ax @ gamma.t()
    if inverse:
        y, dd, dn = x * n, g * n, g * x
    else:
        dd = g / n
        y, dn = x / n, -dd * x / n
    t = dn @ gb                                                                    # t[m, j] = sum_i gamma[i, j] dn[m, i]
    return dict(n=n, y=y, dd=dd, d_norm=dn, t=t, dx=dd + sign(x) * t, d_beta=dn.sum(0), d_gamma=dn.t() @ ax)


def reference_of(c, **kw):
    return reference(c['x'], c['g'], c['gamma'], c['beta'], c['inverse'], **kw)


# --------------------------------------------------------------------------------------------- #
# comparison
# --------------------------------------------------------------------------------------------- #
def round_to(ref64, dtype):
    return ref64.to(F32).to(dtype)


def cast(ref64, dtype):
    """The ONE rounding of an exact reference to the kernel's output type."""
    f32 = ref64.to(F32)
    assert torch.equal(f32.to(F64), ref64), 'the reference is not exact in f32'
    return f32.to(dtype)


def differing(got, want):
    """Mask of the elements of `got` (bf16 / f32) that differ from `want` (the cast reference, same dtype) or are not finite."""
    assert got.dtype == want.dtype and got.numel() == want.numel(), (got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    gd = got.reshape(want.shape).to(F64)
    return (gd != want.to(F64)) | ~torch.isfinite(gd)


def assert_same(got, want, what, unit_rows=None):
    """No element differs; on failure: how many, the first, and which rows / units / channels / channel quads the mismatches span."""
    bad = differing(got, want)
    n = int(bad.sum())
    if n == 0:
        return 0
    idx = bad.nonzero().cpu()
    first = tuple(int(v) for v in idx[0])
    lines = ['{}: {} of {} elements differ'.format(what, n, bad.numel()),
             'first at {}: got {!r}, want {!r}'.format(first, got.reshape(want.shape)[first].item(), want[first].item())]
    if idx.shape[1] == 2:
        for name, v, group in (('pixel', idx[:, 0], 1), ('unit', idx[:, 0], unit_rows or 1), ('row in 16', idx[:, 0] % 16, 1),
                               ('channel', idx[:, 1], 1), ('channel quad', idx[:, 1], 4), ('channel // 16', idx[:, 1], 16)):
            u = torch.unique(v // group)
            lines.append('{}: {} distinct, {}..{}'.format(name, u.numel(), int(u.min()), int(u.max())))
    raise AssertionError('\n  '.join(lines))


# --------------------------------------------------------------------------------------------- #
# exactness conditions
# --------------------------------------------------------------------------------------------- #
def _multiple(v, q):
    return bool((torch.round(v / q) * q == v).all())


def _bf16_exact(v):
    return torch.equal(v.to(F32).to(BF).to(F64), v)


def check_exactness(c, chunk=8192):
    """Every condition under which a correct kernel equals cast(reference), proven on the reference of case c, `chunk` rows at a
    time -> the largest sum of |terms| / quantum met, per sum."""
    x, g, gamma, beta = (c[k].to(F64) for k in ('x', 'g', 'gamma', 'beta'))
    M, C = x.shape
    kind = c['kind']
    for t in (c['x'], c['g'], c['gamma'], c['beta']):
        assert torch.equal(t.to(BF).to(F32), t), 'operands must be exact in bf16'
    if kind == 'div':
        s = c['s'].to(F64)
        q_n, q_dn = s / 1.0, 1.0 / (s * s * 256.0)        # per column: n = s * 2^k, k <= 4; dn = -g x / (s^2 4^k)
        q_t = 2.0 ** -11                                  # gamma (1/2) * dn (2^-10); dd = g / n: multiples of 2^-5
    else:
        q_n, q_dn, q_t = 0.5, 1.0, 0.5
    worst = dict(gemm1=0.0, gemm2=0.0, d_beta=0.0)
    col = torch.zeros(C, dtype=F64)
    ag = gamma.abs()
    for m0 in range(0, M, chunk):
        sl = slice(m0, min(M, m0 + chunk))
        r = reference(x[sl], g[sl], gamma, beta, c['inverse'])
        if kind == 'div':
            mant, _ = torch.frexp(r['n'])
            assert bool((mant == 0.5).all()), 'a norm is not a power of two'
            assert float((r['n'] / c['s'].to(F64)).max()) <= 16.0
        assert _multiple(r['n'], q_n) and _multiple(r['d_norm'], q_dn) and _multiple(r['dd'], q_t) and _multiple(r['t'], q_t)
        # GEMM 1 (+ beta): all terms are positive, their sum is n
        worst['gemm1'] = max(worst['gemm1'], float((r['n'] / q_n).max()))
        # GEMM 2 on top of sign(x) dd, and the last addition
        worst['gemm2'] = max(worst['gemm2'], float(((r['d_norm'].abs() @ ag + r['dd'].abs()) / q_t).max()))
        col += r['d_norm'].abs().sum(0) / q_dn
        assert _bf16_exact(r['d_norm']), 'd_norm is not exact in bf16: GEMM 2 would run on a rounded operand'
        if kind != 'wide':
            assert _bf16_exact(r['dd'][x[sl] == 0]), 'a parked dd is not exact in bf16'
        for k in ('y', 'dx', 'dd', 'd_norm', 'n'):
            assert torch.equal(r[k].to(F32).to(F64), r[k]), k + ' is not exact in f32'
        if kind == 'narrow':
            for k in ('y', 'dx', 'd_norm'):
                assert float(r[k].abs().max()) <= NARROW_QUANTA * 0.5, 'narrow: max |{}| = {}'.format(k, float(r[k].abs().max()))
    worst['d_beta'] = float(col.max())
    for k, v in worst.items():
        assert v < EXACT_LIMIT, '{}: sum of |terms| / quantum = {} >= 2^24'.format(k, v)
    return worst


def check_zeros(c, cus):
    """The zero plan is in the operands, and g != 0 at every zero of x and in the whole last row."""
    x, g, plan = c['x'], c['g'], c['plan']
    M, C = x.shape
    L = launch(C, M, cus)
    zero = x == 0
    if plan['pixel'] is not None:
        assert bool(zero[plan['pixel']].all())
    else:
        assert M < 3
    assert bool(zero[:, plan['channel']].all()) and bool(zero[plan['last']]) and plan['last'][0] == M - 1
    nz = plan['neg_zero']
    assert float(x[nz]) == 0.0 and bool(torch.signbit(x[nz])) and int((torch.signbit(x) & zero).sum()) == 1
    assert (plan['second'] is not None) == (L['trips'] > 1)
    if plan['second'] is not None:
        for pos in plan['second']:
            assert bool(zero[pos]) and L['second_trip_row'] <= pos[0] < min(M, L['second_trip_row'] + UNIT_ROWS[C])
    assert bool((g[zero] != 0).all()) and bool((g[M - 1] != 0).all())
    if M > 1:
        assert int(zero.sum()) >= max(C, int(0.009 * M * C)) and not bool(zero[0].all())
    assert not bool(zero[M - 1].all())
