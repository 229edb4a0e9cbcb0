"""Plain-torch reference of the batch-norm training kernels (sc2_bn_train_fwd / sc2_bn_train_bwd, csrc/bn.hip), working from the
KERNELS' operands as include/sc2_bottleneck.h states them: x, residual, dy, y as [M, C] (bf16 values held in a wider dtype), gamma,
beta, running_mean, running_var as f32 [C], momentum, eps, relu.  It runs in the dtype it is built with:

  float64  the reference tests/test_gpu_bn_train.py compares the kernels with: two-pass variance, the contract's formulas as written
           (tests/test_bn_ref_cpu.py proves it against torch.native_batch_norm + autograd in float64);
  float32  the same contract at the kernel's precision and in the algebraic form csrc/bn.hip documents: one pass for sum x and
           sum x^2, variance = E[x^2] - mean^2 clamped at 0, y = x * scale + shift, dx = ca dz + cb x + cc.  Its sums run in a
           fixed pairwise order made of element-wise f32 additions, and sqrt / division are correctly rounded, so the figures below
           are the same bits on every host and thread count.  This form is the YARDSTICK: its error against the float64 form,
           under the metrics of this file, is what f32 arithmetic costs this algorithm.  The GPU test's slack is F32_MARGIN times it.

Backward: the ReLU mask comes from the y that is passed in (the kernel's contract), never from a recomputed forward, so every element
is decidable and no case excludes elements.
"""
import torch

BN_THREADS, BN_UNROLL = 512, 2          # csrc/bn.hip
STREAM_THREADS, STREAM_GRID_CAP = 256, 8192
FIN_CHANNELS, FIN_SLICES = 32, 8        # the finalize kernels: 32 channels x 8 slices per workgroup

# (C, M, cpr, ppi, idle threads, nb) -- what each case reaches: docstring of tests/test_gpu_bn_train.py
CASES = (
    (8, 2, 1, 512, 0, 1),
    (24, 1361, 3, 170, 2, 2),
    (128, 2049, 16, 32, 0, 9),
    (40, 19585, 5, 102, 2, 25),
    (72, 14337, 9, 56, 8, 33),
    (1032, 100, 129, 3, 125, 5),
    (2040, 37, 255, 2, 2, 3),
    (2048, 8200, 256, 2, 0, 512),
)
COMBOS = ((False, False), (False, True), (True, False), (True, True))       # (relu, residual)
ALT = dict(momentum=0.25, eps=1e-3)      # the second parameter set, on the C = 24 case
NAN_CHANNEL = 3

# float32-form error against the float64 form under the metrics below: the maximum over every case of CASES (default momentum / eps,
# plus ALT on C = 24) and the four (relu, residual) combinations.  Per-case values: docstring of tests/test_bn_ref_cpu.py, which
# re-measures them and fails if one exceeds its constant.  The GPU test's slack is F32_MARGIN times these -- never anything measured
# on the kernel.
E_F32_MAX = {
    'y': 1.11e-6,                # at C = 72
    'dx': 7.58e-7,               # at C = 2048
    'save_mean': 1.56e-7,        # at C = 2048
    'save_rstd': 1.08e-6,        # at C = 72
    'running_mean': 1.36e-7,     # at C = 2048
    'running_var': 1.19e-7,      # at C = 1032
    'dbeta': 2.46e-8,            # at C = 2040
    'dgamma': 5.85e-7,           # at C = 2040
}
F32_MARGIN = 8.0
BF16_ROUND = 2.0 ** -8                   # the single bf16 rounding a bf16 output is allowed, relative to the reference


def launch(M, C):
    """The launcher's arithmetic of csrc/bn.hip restated: dict(cpr, ppi, idle, nb, ws_floats, chunks, stream_blocks, stream_trips,
    fin_blocks, fin_live_last, and the trips of slice 0 of bn_sum_partials through its unrolled loop and its tail: unrolled_trips, tail_trips)."""
    assert M > 0 and C > 0 and C % 8 == 0 and C // 8 <= 256
    cpr = C // 8
    ppi = BN_THREADS // cpr
    nb = min(max(-(-M // (ppi * BN_UNROLL * 4)), 1), 512)
    chunks = M * cpr
    stream_blocks = min(-(-chunks // STREAM_THREADS), STREAM_GRID_CAP)
    fin_blocks = -(-C // FIN_CHANNELS)
    b, unrolled = 0, 0                                   # slice 0 of bn_sum_partials
    while b + 24 < nb:
        b, unrolled = b + 32, unrolled + 1
    tail = len(range(b, nb, FIN_SLICES))
    return dict(cpr=cpr, ppi=ppi, idle=BN_THREADS - ppi * cpr, nb=nb, ws_floats=nb * 2 * C + 3 * C, chunks=chunks,
                stream_blocks=stream_blocks, stream_trips=-(-chunks // (stream_blocks * STREAM_THREADS)), fin_blocks=fin_blocks,
                fin_live_last=C - FIN_CHANNELS * (fin_blocks - 1), unrolled_trips=unrolled, tail_trips=tail)


def bf16(t):
    """t rounded to bf16, held in t's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def make_case(C, M, seed=None):
    """Seeded operands of one case, f32 tensors; x, residual, dy bf16-representable.  Channel c of x is sigma_c N(0, 1) + mu_c with
    sigma spread over [0.5, 2] and mu over [-2, 2], all different; channel 1 has mu = 4 sigma, channel 2 is the constant 0.5, a few
    elements are exact zeros.  gamma in +-[0.5, 1.5] (both signs), beta in [-0.5, 0.5], running statistics random."""
    seed = C * 100003 + M if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    sigma = torch.linspace(0.5, 2.0, C)[torch.randperm(C, generator=g)]
    mu = torch.linspace(-2.0, 2.0, C)[torch.randperm(C, generator=g)]
    mu[1] = 4.0 * sigma[1]
    x = torch.randn(M, C, generator=g) * sigma + mu
    x[:, 2] = 0.5
    zeros = [((k * 7919 + 1) % M, 4 + k % (C - 4)) for k in range(5)]
    for r, c in zeros:
        x[r, c] = 0.0
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma[0], gamma[NAN_CHANNEL] = gamma[0].abs(), -gamma[NAN_CHANNEL].abs()
    beta = torch.rand(C, generator=g) - 0.5
    running_mean = torch.randn(C, generator=g)
    running_var = 0.5 + 1.5 * torch.rand(C, generator=g)
    residual = torch.randn(M, C, generator=g)
    dy = torch.randn(M, C, generator=g)
    return dict(C=C, M=M, x=bf16(x), residual=bf16(residual), dy=bf16(dy), gamma=gamma, beta=beta, running_mean=running_mean,
                running_var=running_var, zeros=zeros)


def _tree_sum(t):
    """Sum over dim 0 in a fixed pairwise order built from element-wise additions (the same bits on every host)."""
    while t.shape[0] > 1:
        n = t.shape[0]
        h = n // 2
        s = t[:h] + t[h:2 * h]
        t = torch.cat([s, t[2 * h:]], 0) if n % 2 else s
    return t[0]


class BnRef:
    """The statistics of (x, gamma, beta, running_*, momentum, eps) in `dtype`; forward() and backward() may be called for several
    (relu, residual) and (dy, y).  Inputs are cloned before conversion (.to(dtype) returns the same tensor when the dtype matches)."""

    def __init__(self, x, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, dtype=torch.float64):
        assert dtype in (torch.float64, torch.float32) and x.dim() == 2 and x.shape[0] > 1
        assert (running_mean is None) == (running_var is None)
        self.dtype = dtype
        conv = self.conv = lambda t: None if t is None else t.detach().clone().to(dtype)
        self.x, self.gamma, self.beta = conv(x), conv(gamma), conv(beta)
        self.M = x.shape[0]
        # M as a tensor beside x: dividing a device tensor by a Python number or a 0-dim CPU tensor multiplies by a rounded 1 / M
        # there, and the constant channel's mean would miss 0.5 by an ulp
        M = self.m = torch.full((1,), float(self.M), dtype=dtype, device=x.device)
        x = self.x
        if dtype == torch.float64:
            self.mean = x.sum(0) / M
            self.var = ((x - self.mean) ** 2).sum(0) / M
            self.var_single_pass = (x * x).sum(0) / M - self.mean ** 2          # (the CPU test asserts the two agree)
        else:
            inv_m = torch.ones_like(M) / M
            self.mean = _tree_sum(x) * inv_m
            self.var = self.var_single_pass = _tree_sum(x * x) * inv_m - self.mean * self.mean
        self.var = self.var.clamp_min(0)
        self.rstd = 1.0 / torch.sqrt(self.var + eps)
        self.running_mean = self.running_var = None
        if running_mean is not None:
            unbiased = self.var * (M / (M - 1.0))
            self.unbiased = unbiased
            self.running_mean = (1.0 - momentum) * conv(running_mean) + momentum * self.mean
            self.running_var = (1.0 - momentum) * conv(running_var) + momentum * unbiased

    def forward(self, relu, residual=None):
        """-> dict(mean, rstd, y (unrounded), pre (y before the ReLU), running_mean, running_var)."""
        if self.dtype == torch.float64:
            pre = (self.x - self.mean) * self.rstd * self.gamma + self.beta
        else:
            scale = self.gamma * self.rstd
            pre = self.x * scale + (self.beta - self.mean * scale)
        if residual is not None:
            pre = pre + self.conv(residual)
        y = torch.relu(pre) if relu else pre
        return dict(mean=self.mean, rstd=self.rstd, y=y, pre=pre, running_mean=self.running_mean, running_var=self.running_var)

    def backward(self, dy, y=None):
        """y: the tensor handed to the kernel (the forward's bf16 output when it applied the ReLU), or None.
        -> dict(dz, dbeta, dgamma, dx)."""
        dy = self.conv(dy)
        dz = dy if y is None else torch.where(self.conv(y) > 0, dy, torch.zeros_like(dy))
        xhat = (self.x - self.mean) * self.rstd
        M = self.m
        if self.dtype == torch.float64:
            dbeta = dz.sum(0)
            dgamma = (dz * xhat).sum(0)
            dx = self.gamma * self.rstd * (dz - dbeta / M - xhat * dgamma / M)
        else:
            inv_m = torch.ones_like(M) / M
            dbeta = _tree_sum(dz)
            dgamma = _tree_sum(dz * xhat)
            ca = self.gamma * self.rstd
            cb = -ca * self.rstd * dgamma * inv_m
            cc = -ca * dbeta * inv_m - cb * self.mean
            dx = ca * dz + cb * self.x + cc
        return dict(dz=dz, dbeta=dbeta, dgamma=dgamma, dx=dx)


# ---- the metrics: every error is taken relative to the natural condition scale of its output (float64, from the reference) ----

def scales_fwd(ref, case_residual, momentum=0.1):
    """ref: a float64 BnRef.  -> dict of condition scales: y [M, C] = the magnitudes of the terms y is summed from; save_mean = rms(x_c);
    save_rstd = rstd_c; running_* = the new value's magnitude plus the update's own scale (momentum x rms(x_c), resp. momentum x the
    unbiased factor x E[x_c^2]: the variance is a difference of two terms of that size)."""
    x, M = ref.x, ref.M
    a = ref.gamma.abs() * ref.rstd
    ex2 = (x * x).sum(0) / M
    s = dict(y=a * (x.abs() + ref.mean.abs()) + ref.beta.abs() + (0 if case_residual is None else case_residual.double().abs()),
             save_mean=ex2.sqrt(), save_rstd=ref.rstd)
    if ref.running_mean is not None:
        s['running_mean'] = ref.running_mean.abs() + momentum * ex2.sqrt()
        s['running_var'] = ref.running_var.abs() + momentum * ex2 * (M / (M - 1.0))
    return s


def scales_bwd(ref, out):
    """out: ref.backward(...) of a float64 BnRef.  dbeta = sum |dz|; dgamma = sum |dz xhat|; dx [M, C] = the magnitudes of the terms
    of gamma rstd (dz - dbeta / M - xhat dgamma / M), with the sums' own scales in place of the sums and |x| + |mean| in place of
    |x - mean| (the kernel forms cb x + cc)."""
    xhat = (ref.x - ref.mean) * ref.rstd
    sb = out['dz'].abs().sum(0)
    sg = (out['dz'] * xhat).abs().sum(0)
    a = ref.gamma.abs() * ref.rstd
    dx = a * (out['dz'].abs() + sb / ref.M + ref.rstd * (ref.x.abs() + ref.mean.abs()) * sg / ref.M)
    return dict(dbeta=sb, dgamma=sg, dx=dx)


def _ratio(d, scale):
    """max d / scale; where the scale is zero (every term of the output is zero: the constant channel's dgamma, a fully masked
    channel) the output has to be exact."""
    scale = scale.double().expand_as(d)
    assert bool((scale >= 0).all())
    r = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float('inf'))))
    return r.max().item()


def err(got, want, scale):
    """max |got - want| / scale over the elements (float64); a NaN or inf anywhere in got gives inf."""
    d = (got.double() - want.double()).abs()
    if not bool(torch.isfinite(d).all()):
        return float('inf')
    return _ratio(d, scale)


def err_bf16(got, want, scale):
    """For a bf16 output: max over the elements of (|got - want| - 2^-8 |want|)+ / scale -- what is left of the error once the one
    permitted rounding is taken off.  The float32 form is not rounded and is measured with err()."""
    d = (got.double() - want.double()).abs()
    if not bool(torch.isfinite(d).all()):
        return float('inf')
    return _ratio((d - BF16_ROUND * want.double().abs()).clamp_min(0), scale)


def variants():
    """Every (C, M, momentum, eps) the calibration and the GPU test run."""
    out = [(C, M, 0.1, 1e-5) for C, M, *_ in CASES]
    out.insert(2, (24, 1361, ALT['momentum'], ALT['eps']))
    return out


def f32_error(case, momentum=0.1, eps=1e-5):
    """The float32 form's error against the float64 form on one case: dict output -> the maximum over the four combinations."""
    args = (case['x'], case['gamma'], case['beta'], case['running_mean'], case['running_var'], momentum, eps)
    r64, r32 = BnRef(*args), BnRef(*args, dtype=torch.float32)
    worst = {k: 0.0 for k in E_F32_MAX}
    for relu, res in COMBOS:
        residual = case['residual'] if res else None
        f64, f32 = r64.forward(relu, residual), r32.forward(relu, residual)
        sc = scales_fwd(r64, residual, momentum)
        for k in ('y', 'save_mean', 'save_rstd', 'running_mean', 'running_var'):
            kk = k[5:] if k.startswith('save_') else k
            worst[k] = max(worst[k], err(f32[kk], f64[kk], sc[k]))
        y = bf16(f64['y']) if relu else None
        b64, b32 = r64.backward(case['dy'], y), r32.backward(case['dy'], y)
        assert torch.equal(b32['dz'].double(), b64['dz'])
        sc = scales_bwd(r64, b64)
        for k in ('dx', 'dbeta', 'dgamma'):
            worst[k] = max(worst[k], err(b32[k], b64[k], sc[k]))
    return worst
