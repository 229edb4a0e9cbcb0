"""Plain-torch reference of the entropy bottleneck's element-wise kernels (sc2_eb_forward / sc2_eb_backward), working from the
KERNEL'S operands: the [C, 64] effective-parameter block (include/sc2_bottleneck.h, "Per-channel parameter block"), y and
noise as [N, C, HW], the mode and lik_bound.  It runs in the dtype it is built with: float64 is the reference the GPU test
compares the kernel with, float32 is the same arithmetic at the kernel's precision -- the yardstick the test's bound is
calibrated on (tests/test_eb_ref_cpu.py proves the float64 form against oracle.cpu_ref.EntropyBottleneck and records the
float32 form's error).

Backward: torch autograd through the forward with respect to y and the block.  CompressAI's LowerBound gate is applied to the
upstream likelihood gradient (it passes where raw >= bound or g_lik < 0).  The kernel's contract in dequantize mode falls out
of the graph: y_hat = round(y - median) + median has no gradient to y (d y = 0) and gradient 1 to the median, so d y_hat is
summed into slot 58.
"""
import torch

NOISE, DEQUANTIZE = 0, 1
STRIDE = 64
N_SLOTS = 59                      # 58 MLP parameters + the median; slots 59..63 are padding (zero)

# The launch shapes of tests/test_gpu_eb_backward.py: (N, C, HW), planes per workgroup, partial rows per plane.
CASES = (
    ((2, 24, 49), 1, 1),          # the only shape the model-level tests reach
    ((33, 32, 70), 1, 1),         # odd N forces 1 although N * C >= 1024; HW no multiple of 64
    ((44, 24, 9), 2, 1),          # HW < one wave: a workgroup's 256 elements span planes
    ((12, 192, 5), 4, 1),         # 8 does not divide N
    ((16, 128, 5), 4, 1),         # 8 leaves fewer than 512 workgroups
    ((32, 128, 5), 8, 1),         # the bs-256 path
    ((2, 6, 1089), 1, 2),         # ragged second row
    ((8, 128, 1030), 2, 2),       # both at once, about 1 M elements
    ((3, 5, 1025), 1, 2),         # odd C, one element in the last row
)
BOUNDS = (1e-9, 0.0)              # every case
BOUND_GATE = 1e-2                 # a real share of elements under the bound: these cases only (ppw 2, 8, 1 x two rows)
GATE_CASES = ((44, 24, 9), (32, 128, 5), (2, 6, 1089))
MAX_MOVED = 0.01                  # cap on the share of elements make_decidable may move

# float32-CPU error of this reference against its float64 form under the GPU test's two metrics, the maximum over every case, mode,
# gradient combination and bound (per-case values: docstring of tests/test_eb_ref_cpu.py, which re-measures them and fails if one
# exceeds these).  The GPU test's bound is F32_MARGIN times these -- never anything measured on the kernel.
E_Y_F32_MAX = 5.62e-6          # at 44 x 24 x 9
E_P_F32_MAX = 1.03e-4          # at 44 x 24 x 9
F32_MARGIN = 8.0


def _slot(P, k):
    return P[:, k].view(1, -1, 1)


def logits(v, P):
    """Cumulative logits L(v) of every element; v [N, C, HW], P [C, 64]."""
    h = [_slot(P, k) * v + _slot(P, 3 + k) for k in range(3)]
    h = [h[k] + _slot(P, 6 + k) * torch.tanh(h[k]) for k in range(3)]
    for layer in range(3):
        q = 9 + 15 * layer
        g = [_slot(P, q + 3 * k) * h[0] + _slot(P, q + 3 * k + 1) * h[1] + _slot(P, q + 3 * k + 2) * h[2] + _slot(P, q + 9 + k)
             for k in range(3)]
        h = [g[k] + _slot(P, q + 12 + k) * torch.tanh(g[k]) for k in range(3)]
    return _slot(P, 54) * h[0] + _slot(P, 55) * h[1] + _slot(P, 56) * h[2] + _slot(P, 57)


class EbRef:
    """One evaluation graph of (P, y, noise, mode) in `dtype`; forward() and backward() may be called for several bounds and
    upstream gradients.  The inputs are cloned and converted with .double() / .float() on the clones: .to(dtype) returns the
    SAME tensor when the dtype already matches, and .grad would then accumulate across instances."""

    def __init__(self, P, y, noise, mode, dtype=torch.float64):
        conv = (lambda t: t.detach().clone().double()) if dtype == torch.float64 else (lambda t: t.detach().clone().float())
        assert dtype in (torch.float64, torch.float32) and mode in (NOISE, DEQUANTIZE)
        self.mode = mode
        self.P = conv(P).requires_grad_(True)
        self.y = conv(y).requires_grad_(True)
        assert self.P.shape == (self.y.shape[1], STRIDE) and self.y.dim() == 3
        if mode == NOISE:
            self.y_hat = self.y + conv(noise)
        else:
            med = _slot(self.P, 58)
            self.y_hat = torch.round(self.y - med) + med
        half = 0.5
        self.raw = torch.sigmoid(logits(self.y_hat + half, self.P)) - torch.sigmoid(logits(self.y_hat - half, self.P))

    def forward(self, lik_bound):
        """-> (y_hat, raw likelihood, bounded likelihood, -log2 bits), detached."""
        raw = self.raw.detach()
        lik = raw.clamp_min(lik_bound)
        return self.y_hat.detach(), raw, lik, -torch.log2(lik)

    def gate(self, lik_bound, g_lik):
        """True where CompressAI's LowerBound lets g_lik through."""
        return (self.raw.detach() >= lik_bound) | (g_lik < 0)

    def backward(self, lik_bound, g_yhat=None, g_lik=None):
        """-> (g_y like y, g_params [C, 64]) for the upstream gradients given (None = zero)."""
        outs, grads = [], []
        if g_yhat is not None:
            outs.append(self.y_hat)
            grads.append(g_yhat.to(self.y.dtype))
        if g_lik is not None:
            g = g_lik.to(self.y.dtype)
            outs.append(self.raw)
            grads.append(torch.where(self.gate(lik_bound, g), g, torch.zeros_like(g)))
        if not outs:
            return torch.zeros_like(self.y), torch.zeros_like(self.P)
        g_y, g_p = torch.autograd.grad(outs, [self.y, self.P], grads, retain_graph=True, allow_unused=True)
        g_y = torch.zeros_like(self.y) if g_y is None else g_y
        g_p = torch.zeros_like(self.P) if g_p is None else g_p
        return g_y.detach(), g_p.detach()


def undecidable(P, y, noise, bounds):
    """Elements on which a correct f32 evaluation may legitimately disagree with float64, in either mode: the float64 raw likelihood
    within 1e-6 of a bound (in f32 the right tail's sigmoid(upper) - sigmoid(lower) is a difference of two numbers near 1, quantum
    about 6e-8: which side of the bound it falls on -- the gate -- is not defined there), or, for the dequantize mode, y - median
    within 1e-4 of a half-integer (the rounding direction)."""
    bad = torch.zeros(y.shape, dtype=torch.bool)
    with torch.no_grad():
        for mode in (NOISE, DEQUANTIZE):
            raw = EbRef(P, y, noise, mode).raw
            for b in bounds:
                bad |= (raw - b).abs() <= 1e-6
        d = y.double() - _slot(P.double(), 58)
        bad |= ((d - torch.floor(d)) - 0.5).abs() <= 1e-4
    return bad


def make_decidable(P, y, noise, bounds):
    """-> (y with every undecidable element moved to its channel's median, the share of elements moved).  At the median both
    modes sit at the density's peak and y - median = 0 rounds to 0; the result is checked to be decidable everywhere."""
    bad = undecidable(P, y, noise, bounds)
    med = P[:, 58].to(y.dtype).view(1, -1, 1).expand_as(y)
    y2 = torch.where(bad, med, y).contiguous()
    assert not bool(undecidable(P, y2, noise, bounds).any()), 'an element is still undecidable at its median'
    return y2, bad.double().mean().item()


def perturbed_oracle(R, C, seed, likelihood_bound=1e-9):
    """The oracle bottleneck with realistic, all-different parameters: its own initialisation, perturb_quantiles (channel-dependent
    medians), 0.3 N(0, 1) on the factors (zero at initialisation: tanh(factor) = 0 would switch every tanh term off) and 0.1 N(0, 1) on
    the matrices (all entries of a layer are equal at initialisation, which would hide a transposed matrix)."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)                      # (the oracle draws its biases from the global generator)
    eb = R.EntropyBottleneck(C, likelihood_bound=likelihood_bound)
    R.perturb_quantiles(eb)
    with torch.no_grad():
        for f in eb.factors:
            f.add_(0.3 * torch.randn(f.shape, generator=g))
        for m in eb.matrices:
            m.add_(0.1 * torch.randn(m.shape, generator=g))
    return eb


def make_case(S, R, shape, seed=None):
    """The operands of one launch shape, every tensor f32 (hence f32-representable): the block of a perturbed oracle bottleneck through
    S.EntropyBottleneck.effective_params(), y = an even mix of 4 N(0, 1) (the bulk) and 24 N(0, 1) (both tails, so that at lik_bound
    1e-2 a real share of elements lies under the bound), made decidable for every bound the tests use; U(-1/2, 1/2) noise; N(0, 1)
    upstream gradients.  -> dict(eb=the oracle module, P, y, noise, g_yhat, g_lik, moved)."""
    N, C, HW = shape
    seed = N * 1000003 + C * 1009 + HW if seed is None else seed
    eb = perturbed_oracle(R, C, seed)
    m = S.EntropyBottleneck(C)
    m.load_state_dict({k: v.clone() for k, v in eb.state_dict().items()})
    with torch.no_grad():
        P = m.effective_params().detach().clone()
    g = torch.Generator().manual_seed(seed + 1)
    wide = torch.rand(N, C, HW, generator=g) < 0.5
    y = torch.randn(N, C, HW, generator=g) * torch.where(wide, torch.tensor(24.0), torch.tensor(4.0))
    noise = torch.rand(N, C, HW, generator=g) - 0.5
    y, moved = make_decidable(P, y, noise, BOUNDS + (BOUND_GATE,))
    g_yhat = torch.randn(N, C, HW, generator=g)
    g_lik = torch.randn(N, C, HW, generator=g)
    return dict(eb=eb, P=P, y=y, noise=noise, g_yhat=g_yhat, g_lik=g_lik, moved=moved)


def e_y(got, ref):
    """max |g_y - ref| / max |ref| (0 / 0 = 0: an all-zero reference wants exact zeros, which the caller asserts)."""
    den = ref.abs().max().item()
    num = (got.double() - ref.double()).abs().max().item()
    return num / den if den > 0 else (0.0 if num == 0 else float('inf'))


def e_p(got, ref):
    """max over channels (rows) of max_k |g[c, k] - ref[c, k]| / max_k |ref[c, k]| over the columns given -- the caller passes slots
    0..58 of the block's gradient; a channel whose reference row is all zero wants an all-zero row."""
    got, ref = got.double(), ref.double()
    num = (got - ref).abs().amax(dim=1)
    den = ref.abs().amax(dim=1)
    e = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float('inf'))))
    return e.max().item()


COMBOS = ('yhat', 'lik', 'both')


def upstream(case, combo):
    return (case['g_yhat'] if combo in ('yhat', 'both') else None, case['g_lik'] if combo in ('lik', 'both') else None)


def bounds_of(shape):
    return BOUNDS + ((BOUND_GATE,) if tuple(shape) in GATE_CASES else ())


def f32_error(case, shape):
    """(E_y, E_p) of the float32 form of this reference against its float64 form: the maximum over both modes, the gradient
    combinations and the bounds of `shape`."""
    worst_y = worst_p = 0.0
    for mode in (NOISE, DEQUANTIZE):
        r64 = EbRef(case['P'], case['y'], case['noise'], mode)
        r32 = EbRef(case['P'], case['y'], case['noise'], mode, torch.float32)
        for bound in bounds_of(shape):
            for combo in COMBOS:
                gy64, gp64 = r64.backward(bound, *upstream(case, combo))
                gy32, gp32 = r32.backward(bound, *upstream(case, combo))
                worst_y = max(worst_y, e_y(gy32, gy64))
                worst_p = max(worst_p, e_p(gp32[:, :N_SLOTS], gp64[:, :N_SLOTS]))
    return worst_y, worst_p
