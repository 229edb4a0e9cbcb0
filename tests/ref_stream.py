"""Plain-torch references of the streaming kernels -- csrc/loss.hip (sc2_mse_sum_bf16, sc2_mse_grad_bf16, sc2_relu_bwd_bf16,
sc2_relu_bwd_mse_bf16), csrc/gdn_bwd.hip (sc2_gdn_bwd_pre, sc2_gdn_bwd_post, sc2_colsum_bf16) and the two conversions of
csrc/layout.hip -- one function per entry point, the formulas as the kernels' header comments state them, in the dtype they are called
with:

  float64  the reference tests/test_gpu_stream_kernels.py holds the kernels against (tests/test_stream_ref_cpu.py proves it against
           torch autograd where autograd states the same thing);
  float32  the same formulas at the kernels' precision and in the order of operations the kernels document (r = 1 / norm once,
           s = 2 scale once, a thread's own chunks added one after the other and the threads in a fixed pairwise order, element-wise f32
           operations throughout: the same bits on every host).  Its error against the float64 form under the metrics of ref_bn.py is
           the YARDSTICK: E_F32_MAX, measured and re-measured by the CPU test; the GPU test's slack is F32_MARGIN times it.

launch(kind, ...) restates the grid arithmetic of each launcher (cpr, ppi, idle threads, workgroups, trips, who is live in the last
one); the GPU test holds it against what the library reports (sc2_mse_partial_len, sc2_gdn_bwd_pre_blocks, sc2_colsum_blocks,
sc2_gdn_bwd_post_blocks, sc2_layout_blocks), so the case tables below stay tied to the launchers.

Operands come in two kinds: 'dyadic' (small integers, norm in {1, 2}, scale 0.5: every f32 intermediate of the kernels is exact, in any
order of summation and with or without FMA contraction, so every output has to EQUAL the reference) and 'random' (N(0, 1) rounded to
bf16, norm uniform in [0.5, 4]).  What each case reaches: docstring of tests/test_gpu_stream_kernels.py.
"""
import torch

from ref_bn import BF16_ROUND, F32_MARGIN, _tree_sum, bf16, err, err_bf16   # noqa: F401  (the metrics: one definition for both files)

KINDS = ('dyadic', 'random')
LOSS_N8 = (1, 257, 1048576, 1048577, 2097452)
PRE_CASES = ((8, 1), (40, 198), (48, 43009), (48, 86059), (1032, 100), (2040, 37), (2048, 3073))                # (C, M)
COLSUM_CASES = ((8, 1), (40, 1000), (96, 198), (96, 21761), (96, 87140), (2040, 37), (2048, 4101))             # (C, M)
POST_N8 = (1, 257, 2097153)
LAYOUT_CASES = ((3, 5, 6, 10, 8), (2, 9, 3, 7, 12), (2, 3, 5, 5, 16), (5, 3, 1, 838861, 4), (5, 8, 1, 838861, 8))   # (N, C, H, W, Cpad)
LAYOUT_BACK_CASES = ((3, 24, 6, 10), (5, 8, 1, 838861))                                                        # (N, C, H, W)
MSE_VARIANTS = ((True, True), (True, False), (False, True), (False, False))                                    # (g present, relu)
SCALE = {'dyadic': 0.5, 'random': 0.37}

LOSS_THREADS, LOSS_CAP = 256, 4096            # csrc/loss.hip
PRE_THREADS, PRE_CAP, PRE_UNROLL = 256, 1024, 2     # csrc/gdn_bwd.hip
CS_THREADS, CS_CAP, CS_UNROLL = 1024, 256, 4
POST_THREADS, POST_CAP = 256, 8192
LAYOUT_THREADS, LAYOUT_CAP = 256, 16384       # csrc/layout.hip

# float32-form error against the float64 form under the metrics of ref_bn.py (err: |f32 - f64| / scale, scale = the sum of the
# magnitudes of the terms added): the maximum over every case of the tables above, both directions of gdn_bwd_pre and the four
# (g, relu) variants of relu_bwd_mse, on the random operands.  tests/test_stream_ref_cpu.py re-measures them.
E_F32_MAX = {
    'mse_sum': 1.85e-7,          # at n8 = 2 097 452 (24 squares per thread, then the pairwise tree)
    'relu_bwd_mse': 1.13e-7,     # at n8 = 2 097 452
    'd_norm': 2.72e-7,           # forward direction, the large cases
    'dx_direct': 1.14e-7,
    'd_beta': 1.80e-7,           # at C = 8, M = 1: one term per column
    'colsum': 1.66e-8,           # at C = 2040, M = 37
}


def _cdiv(a, b):
    return -(-a // b)


def _clip(v, hi):
    return max(0, min(v, hi))


def launch(kind, *dims):
    """The launchers' arithmetic restated.  'loss' (n) / 'gdn_bwd_post' (n) / 'layout' (pixels): blocks, uncapped (the grid without its
    cap), trips (grid-stride iterations of the busiest thread), last_trip (chunks or pixels the last trip covers).  'gdn_bwd_pre' /
    'colsum' (M, C): cpr, ppi, idle (threads of a workgroup that own no pixel), blocks, uncapped, stride (pixels all workgroups cover
    per unroll slot), iters, last_live (per unroll slot: the threads of the whole grid for which that slot is live in the last
    iteration; slot 1 of gdn_bwd_pre is the kernel's `two`)."""
    if kind in ('loss', 'gdn_bwd_post', 'layout'):
        (n,) = dims
        threads, cap, unit = {'loss': (LOSS_THREADS, LOSS_CAP, 8), 'gdn_bwd_post': (POST_THREADS, POST_CAP, 8),
                              'layout': (LAYOUT_THREADS, LAYOUT_CAP, 1)}[kind]
        assert n > 0 and n % unit == 0
        items = n // unit
        uncapped = _cdiv(items, threads)
        blocks = min(uncapped, cap)
        per = blocks * threads
        trips = _cdiv(items, per)
        return dict(items=items, blocks=blocks, uncapped=uncapped, trips=trips, last_trip=items - (trips - 1) * per)
    M, C = dims
    threads, cap, unroll = {'gdn_bwd_pre': (PRE_THREADS, PRE_CAP, PRE_UNROLL), 'colsum': (CS_THREADS, CS_CAP, CS_UNROLL)}[kind]
    assert M > 0 and C > 0 and C % 8 == 0 and C // 8 <= 256
    cpr = C // 8
    ppi = threads // cpr
    uncapped = _cdiv(M, ppi)
    blocks = min(uncapped, cap)
    stride = blocks * ppi
    iters = _cdiv(M, unroll * stride)
    last_live = tuple(_clip(M - (unroll * (iters - 1) + u) * stride, stride) for u in range(unroll))
    return dict(cpr=cpr, ppi=ppi, idle=threads - ppi * cpr, blocks=blocks, uncapped=uncapped, stride=stride, iters=iters,
                last_live=last_live)


# ---- operands (CPU f32 tensors holding bf16-representable values; seeded) ----

SUB = 2.0 ** -133                      # the smallest positive bf16 subnormal


def _gen(kind, shape, g, lim=4):
    if kind == 'dyadic':
        return torch.randint(-lim, lim + 1, shape, generator=g).float()
    return bf16(torch.randn(shape, generator=g))


def _nonzero(t):
    return torch.where(t == 0, torch.ones_like(t), t)


def make_loss_case(n8, kind):
    """x, y (the MSE pair), g, out, t, add: [8 n8].  The last chunk's x - y is nonzero in its first element (the chunk the last ragged
    trip alone reaches changes its workgroup's partial).  `out` carries +0, -0 in elements 0, 1 of the first and of the last chunk, with
    nonzero g, add and t beside them: a mask of `>= 0` lets a nonzero gradient through there."""
    assert kind in KINDS
    gen = torch.Generator().manual_seed(7 * n8 + KINDS.index(kind))
    n = 8 * n8
    d = {k: _gen(kind, (n,), gen) for k in ('x', 'y', 'g', 'out', 't', 'add')}
    d['x'][n - 8], d['y'][n - 8] = 3.0, -2.0
    for base in (0, n - 8):
        d['out'][base], d['out'][base + 1] = 0.0, -0.0
        for k in ('g', 'add', 't'):
            d[k][base:base + 2] = _nonzero(d[k][base:base + 2])
        d['add'][base:base + 2] = d['g'][base:base + 2]                     # (g + add and g - 2 scale t stay nonzero)
        d['t'][base:base + 2] = -d['g'][base:base + 2]
    d.update(n8=n8, n=n, kind=kind, scale=SCALE[kind])
    return d


def make_pre_case(C, M, kind):
    """gy, x, norm: [M, C]; the last pixel's gy and x are nonzero in every channel (it contributes to every column sum)."""
    assert kind in KINDS
    gen = torch.Generator().manual_seed(C * 100003 + M + KINDS.index(kind))
    gy, x = _gen(kind, (M, C), gen), _gen(kind, (M, C), gen)
    gy[M - 1], x[M - 1] = _nonzero(gy[M - 1]), _nonzero(x[M - 1])
    if kind == 'dyadic':
        norm = torch.randint(1, 3, (M, C), generator=gen).float()
    else:
        norm = bf16(0.5 + 3.5 * torch.rand(M, C, generator=gen))
    return dict(C=C, M=M, kind=kind, gy=gy, x=x, norm=norm)


def make_colsum_case(C, M, kind):
    assert kind in KINDS
    gen = torch.Generator().manual_seed(C * 100019 + M + KINDS.index(kind))
    x = _gen(kind, (M, C), gen, lim=8)
    x[M - 1] = _nonzero(x[M - 1])
    return dict(C=C, M=M, kind=kind, x=x)


POST_X_FIXED = (0.0, -0.0, 2.0, -3.0)       # elements 0..3 of the first and of the last chunk of x


def make_post_case(n8, kind):
    """dx_direct, x, t: [8 n8]; x carries +0, -0, a positive and a negative value at fixed positions of the first and the last chunk,
    t is nonzero there."""
    assert kind in KINDS
    gen = torch.Generator().manual_seed(11 * n8 + KINDS.index(kind))
    n = 8 * n8
    d = {k: _gen(kind, (n,), gen) for k in ('dx_direct', 'x', 't')}
    for base in (0, n - 8):
        d['x'][base:base + 4] = torch.tensor(POST_X_FIXED)
        d['t'][base:base + 4] = _nonzero(d['t'][base:base + 4])
    d.update(n8=n8, n=n, kind=kind)
    return d


def layout_specials():
    """f32 bit patterns for sc2_nchw_f32_to_nhwc_bf16: +-0, +-inf, NaN, f32 subnormals, the largest finite f32 (rounds to inf), one f32
    ulp to either side of a bf16 tie, exact ties on an even and an odd bf16 mantissa (both signs of the odd one)."""
    bits = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001, 0x807FFFFF, 0x007FFFFF, 0x7F7FFFFF, 0xFF7FFFFF,
            0x3F807FFF, 0x3F808001, 0x3F808000, 0x3F818000, 0xBF818000, 0x3F817FFF, 0x3F818001]
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


def make_layout_case(N, C, H, W):
    """x f32 [N, C, H, W], N(0, 1) NOT rounded to bf16 (the kernel rounds), with layout_specials() in the first pixels of image 0 and in
    the last pixels of image N - 1, the last pixel among them -> (x, positions [(n, c, h, w)] of the specials in their order, twice)."""
    gen = torch.Generator().manual_seed(((N * 31 + C) * 31 + H) * 31 + W)
    x = torch.randn(N, C, H, W, generator=gen)
    sp = layout_specials()
    assert len(sp) <= C * H * W
    flat = x.view(N, C, H * W)
    pos = []
    for k in range(len(sp)):
        pos.append((0, k % C, k // C))
    for k in range(len(sp)):
        pos.append((N - 1, C - 1 - k % C, H * W - 1 - k // C))
    for k, (n, c, p) in enumerate(pos):
        flat[n, c, p] = sp[k % len(sp)]
    return x, pos


# ---- the references: float64 by default, dtype=float32 for the yardstick ----

def _f(t, dtype):
    return t.detach().clone().to(dtype)


def by_workgroup(per_chunk, grid):
    """per_chunk [n8, k] -> [trips, grid, 256, k] with zero rows behind the end: workgroup b of a grid g owns the chunks i with
    (i mod 256 g) // 256 == b."""
    n8 = per_chunk.shape[0]
    per = grid * LOSS_THREADS
    trips = _cdiv(n8, per)
    if trips * per != n8:
        per_chunk = torch.cat([per_chunk, per_chunk.new_zeros(trips * per - n8, per_chunk.shape[1])])
    return per_chunk.view(trips, grid, LOSS_THREADS, per_chunk.shape[1])


def mse_sum(x, y, grid, dtype=torch.float64):
    """The per-workgroup partial sums of (x - y)^2 -> [grid].  (Every term is positive: the partial is its own condition scale.)"""
    d = _f(x, dtype) - _f(y, dtype)
    sq = by_workgroup((d * d).view(-1, 8), grid)
    if dtype == torch.float64:
        return sq.sum((0, 2, 3))
    acc = torch.zeros(grid, LOSS_THREADS, dtype=dtype, device=sq.device)       # a thread's own chunks, one element after the other
    for trip in range(sq.shape[0]):
        for k in range(8):
            acc = acc + sq[trip, :, :, k]
    return _tree_sum(acc.t().contiguous())                                      # the 256 threads pairwise


def mse_grad(x, y, scale, dtype=torch.float64):
    return 2.0 * scale * (_f(x, dtype) - _f(y, dtype))


def relu_bwd(g, out, add=None, dtype=torch.float64):
    v = _f(g, dtype) if add is None else _f(g, dtype) + _f(add, dtype)
    return torch.where(_f(out, dtype) > 0, v, torch.zeros_like(v))


def relu_bwd_mse(g, out, t, scale, relu, dtype=torch.float64):
    """([g] + 2 scale (out - t)) [(out > 0)] -> (value, condition scale |g| + 2 |scale| (|out| + |t|))."""
    o, tt = _f(out, dtype), _f(t, dtype)
    s = torch.full((), 2.0, dtype=dtype, device=o.device) * torch.full((), scale, dtype=torch.float32, device=o.device).to(dtype)
    v = s * (o - tt)
    sc = s.abs() * (o.abs() + tt.abs())
    if g is not None:
        v = _f(g, dtype) + v
        sc = sc + _f(g, dtype).abs()
    if relu:
        v = torch.where(o > 0, v, torch.zeros_like(v))
    return v, sc


def gdn_bwd_pre(gy, x, norm, inverse, dtype=torch.float64):
    """-> dict(d_norm, dx_direct (both unrounded), d_beta = the column sums of the unrounded d_norm, d_beta_scale = sum |d_norm|)."""
    g, xv, nv = _f(gy, dtype), _f(x, dtype), _f(norm, dtype)
    if inverse:
        d_norm, dxd = g * xv, g * nv
    elif dtype == torch.float64:
        d_norm, dxd = -g * xv / (nv * nv), g / nv
    else:
        r = torch.ones_like(nv) / nv
        dxd = g * r
        d_norm = -dxd * xv * r
    d_beta = d_norm.sum(0) if dtype == torch.float64 else _tree_sum(d_norm)
    return dict(d_norm=d_norm, dx_direct=dxd, d_beta=d_beta, d_beta_scale=d_norm.abs().sum(0))


def sign(x):
    """d|x| / dx as torch.abs differentiates it: 0 at +-0."""
    one = torch.ones_like(x)
    return torch.where(x > 0, one, torch.where(x < 0, -one, torch.zeros_like(x)))


def gdn_bwd_post(dx_direct, x, t, dtype=torch.float64):
    return _f(dx_direct, dtype) + sign(_f(x, dtype)) * _f(t, dtype)


def colsum(x, dtype=torch.float64):
    """-> (column sums of the bf16 values, condition scale sum |x|)."""
    v = _f(x, dtype)
    return (v.sum(0) if dtype == torch.float64 else _tree_sum(v)), v.abs().sum(0)


def nchw_to_nhwc_bf16(x, cpad):
    """A permute, torch's cast and zero padding -> bf16 [N, H, W, cpad]."""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, cpad, dtype=torch.bfloat16, device=x.device)
    y[..., :C] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    return y


def nhwc_bf16_to_nchw(x):
    return x.permute(0, 3, 1, 2).float().contiguous()


# ---- the yardstick ----

def f32_error_loss(case):
    """dict(mse_sum, relu_bwd_mse) of one random loss case."""
    grid = launch('loss', case['n'])['blocks']
    p64 = mse_sum(case['x'], case['y'], grid)
    out = {'mse_sum': err(mse_sum(case['x'], case['y'], grid, torch.float32), p64, p64), 'relu_bwd_mse': 0.0}
    for has_g, relu in MSE_VARIANTS:
        g = case['g'] if has_g else None
        v64, sc = relu_bwd_mse(g, case['out'], case['t'], case['scale'], relu)
        v32, _ = relu_bwd_mse(g, case['out'], case['t'], case['scale'], relu, torch.float32)
        out['relu_bwd_mse'] = max(out['relu_bwd_mse'], err(v32, v64, sc))
    return out


def f32_error_pre(case):
    out = {'d_norm': 0.0, 'dx_direct': 0.0, 'd_beta': 0.0}
    for inverse in (False, True):
        r64 = gdn_bwd_pre(case['gy'], case['x'], case['norm'], inverse)
        r32 = gdn_bwd_pre(case['gy'], case['x'], case['norm'], inverse, torch.float32)
        out['d_norm'] = max(out['d_norm'], err(r32['d_norm'], r64['d_norm'], r64['d_norm'].abs()))
        out['dx_direct'] = max(out['dx_direct'], err(r32['dx_direct'], r64['dx_direct'], r64['dx_direct'].abs()))
        out['d_beta'] = max(out['d_beta'], err(r32['d_beta'], r64['d_beta'], r64['d_beta_scale']))
    return out


def f32_error_colsum(case):
    s64, sc = colsum(case['x'])
    return {'colsum': err(colsum(case['x'], torch.float32)[0], s64, sc)}
