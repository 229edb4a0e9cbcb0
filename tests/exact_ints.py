"""Integer operands for zero-tolerance kernel checks: test infrastructure only.

Products of small integers are exact in bf16 and in f32, and every partial sum below 2^24 is an exact f32 number in any
summation order -- inside the MFMA's own 32-term sum as well.  A correct bf16 kernel therefore equals the integer convolution
bit for bit, its f32 store equals the f64 result and its bf16 store equals `exact.to(bfloat16)` (round to nearest even,
applied once).  Two operand sets:

  wide    integers uniform in {-3..3}: outputs run into the hundreds, so the rounding of a bf16 store and its ties
          (odd integers in 256..512, ...) are exercised;
  narrow  values in {-1, 0, 1} with the share of non-zeros chosen per K so that K p_x p_w <= 1024: the output's standard
          deviation is at most 32 and `check_narrow` asserts max|ref| <= 256 -- every output is a bf16-exact integer, and one
          missing (or doubled) non-zero term shows even through a bf16 store.

Bias: f32 integers in {-4..4}; residuals: bf16 integers in {-3..3}.  `check_bound` asserts K max|x| max|w| + |bias| + |res| < 2^24
for a case.  References run on the CPU in f64 (F.conv2d, conv_transpose2d, autograd for the weight gradient); the test applies
the kernel's documented epilogue in f64 and `cast` rounds ONCE to the output type.

GDN1 with a live gamma: `gdn_params` draws gamma with three entries from {1/2, 1, 2} per row and column and beta from {1, 2, 3}, so
n = beta + gamma |t| is a multiple of 1/2 and an exact f32 number in any summation order (`gdn_norm` asserts it).  The forward form
r = 1.0f / n, y = t * r is then two correctly rounded f32 operations on exact operands -- the same bits on the CPU as on the device --
and `gdn_restate` is that arithmetic in torch float32, with the precision (f32 accumulator or its bf16 rounding) in which t enters the
second GEMM and the product as parameters.  `gdn_admissible` gives, for the two kernels that multiply by the hardware reciprocal
(within 1 ulp), the bf16 results under r and its two f32 neighbours; `assert_bits_in` compares with such a set.

`arena(t)` puts an operand between two guard bands of NaN (integer types: a large sentinel) inside a larger buffer, so that a
read past an operand -- even one multiplied by a zero weight -- poisons the output, and a write past an output shows in
`bands_untouched`.  Only memory the test owns is read or written."""
import math

import torch
import torch.nn.functional as F

EXACT_LIMIT = 1 << 24
NARROW_MAX = 256
GUARD_BYTES = 1 << 16       # at least 64 KB of fill on each side of an arena view
ALIGN = 256
INT_SENTINEL = {torch.int32: 0x7F5A5A5A, torch.int64: 0x7F5A5A5A5A5A5A5A, torch.int16: 0x7F5A, torch.uint8: 0xA5, torch.int8: 0x5A}
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# --------------------------------------------------------------------------------------------- #
# operands
# --------------------------------------------------------------------------------------------- #
def gen(*seed):
    """A CPU generator seeded from the case's parameters."""
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v)) % (1 << 31)
    return torch.Generator().manual_seed(s)


def wide(shape, g):
    """f32 tensor of integers uniform in {-3..3}."""
    return torch.randint(-3, 4, tuple(shape), generator=g).float()


def wide_amplitude(K):
    """The GDN1 cases' wide set at short K: with {-3..3} a sum of K < 512 products stays a bf16-exact integer (4 sqrt(K) < 90), and
    whether a kernel takes t as its f32 accumulator or rounded to bf16 could not be seen.  Integers up to 8 (K >= 128) or 15 are
    still exact in bf16, their products exact in f32, and the sums reach past 256."""
    return 3 if K >= 512 else 8 if K >= 128 else 15


def narrow_amplitude(K):
    """The GDN1 cases' narrow set at short K: {-1, 0, 1} leaves |t| <= 8 or so at K = 8 .. 100, mostly powers of two, for which
    t * (1 / n) IS the rounded t / n -- the order of operations could not be seen.  The largest a with a (a + 1) sqrt(K) <= 120
    (uniform {-a..a}: std(t) = a (a + 1) sqrt(K) / 3 <= 40, so max|t| <= 256 still holds and is still asserted); 1: the plain set."""
    a = 1
    while (a + 1) * (a + 2) * math.sqrt(max(int(K), 1)) <= 120.0:
        a += 1
    return a


def wide_to(shape, a, g):
    """f32 tensor of integers uniform in {-a..a}."""
    return torch.randint(-int(a), int(a) + 1, tuple(shape), generator=g).float()


def narrow_p(K):
    """Share of non-zeros of EACH operand on the narrow set: p^2 K <= 1024 (and some zeros at every K)."""
    return min(0.75, math.sqrt(1024.0 / max(int(K), 1)))


def narrow(shape, K, g):
    """f32 tensor with values in {-1, 0, 1}, non-zero with probability narrow_p(K)."""
    sign = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    keep = (torch.rand(tuple(shape), generator=g) < narrow_p(K)).float()
    return sign * keep


def operand(kind, shape, K, g):
    assert kind in ('wide', 'narrow')
    return wide(shape, g) if kind == 'wide' else narrow(shape, K, g)


def bias_ints(c, g):
    """f32 integers in {-4..4}."""
    return torch.randint(-4, 5, (int(c),), generator=g).float()


def residual_ints(shape, g):
    """bf16 integers in {-3..3}."""
    return torch.randint(-3, 4, tuple(shape), generator=g).to(torch.bfloat16)


def quarter_medians(c, g):
    """f32 multiples of 0.25 in [-2, 2]: y - median meets exact .5 ties, so round-half-even is exercised."""
    return torch.randint(-8, 9, (int(c),), generator=g).float() * 0.25


def check_bound(K, x, w, bias=None, res=None):
    """Every partial sum of the case is an exact f32 number."""
    mx = float(x.abs().max()) if x.numel() else 0.0
    mw = float(w.abs().max()) if w.numel() else 0.0
    total = int(K) * mx * mw
    total += float(bias.abs().max()) if bias is not None and bias.numel() else 0.0
    total += float(res.float().abs().max()) if res is not None and res.numel() else 0.0
    assert total < EXACT_LIMIT, 'K {} max|x| {} max|w| {}: bound {} >= 2^24'.format(K, mx, mw, total)
    for t in (x, w, bias, res):
        if t is not None:
            assert torch.equal(t.double(), t.double().round()), 'operands must be integers'
            assert torch.equal(t.to(torch.bfloat16).double(), t.double()), 'operands must be exact in bf16'


def check_narrow(ref):
    """The narrow rule: every value of the reference is a bf16-exact integer (|v| <= 256)."""
    m = float(ref.abs().max()) if ref.numel() else 0.0
    assert m <= NARROW_MAX, 'narrow operands gave max|ref| = {} > {}'.format(m, NARROW_MAX)


# --------------------------------------------------------------------------------------------- #
# references (f64, CPU)
# --------------------------------------------------------------------------------------------- #
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv_ref(x, w, stride=1, pad=0, dilation=1):
    """x [N,Cin,H,W], w [Cout,Cin,KH,KW] (integer valued) -> f64 [N,Cout,OH,OW]."""
    return F.conv2d(x.double(), w.double(), None, _pair(stride), _pair(pad), _pair(dilation))


def conv_ref_f32(x, w, stride=1, pad=0, dilation=1):
    return F.conv2d(x.float(), w.float(), None, _pair(stride), _pair(pad), _pair(dilation))


def conv_ref_int(x, w, stride=1, pad=0, dilation=1):
    """The same convolution as an int64 einsum over unfolded windows (slow: small cases; pins conv_ref itself)."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(pad), _pair(dilation)
    xi = F.pad(x.to(torch.int64), (pw, pw, ph, ph))
    wi = w.to(torch.int64)
    N, C, H, W = xi.shape
    Co, _, KH, KW = wi.shape
    OH = (H - dh * (KH - 1) - 1) // sh + 1
    OW = (W - dw * (KW - 1) - 1) // sw + 1
    cols = torch.empty((N, C, KH, KW, OH, OW), dtype=torch.int64)
    for a in range(KH):
        for b in range(KW):
            cols[:, :, a, b] = xi[:, :, a * dh:a * dh + (OH - 1) * sh + 1:sh, b * dw:b * dw + (OW - 1) * sw + 1:sw]
    return torch.einsum('ncabhw,ocab->nohw', cols, wi)


def dgrad_ref(gy, w, stride, pad, in_hw):
    """Data gradient of y = conv2d(x, w, stride, pad): gy [N,Cout,OH,OW] -> f64 [N,Cin,H,W]."""
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    H, W = in_hw
    KH, KW = w.shape[2:]
    oph = H - ((gy.shape[2] - 1) * sh - 2 * ph + KH)
    opw = W - ((gy.shape[3] - 1) * sw - 2 * pw + KW)
    if 0 <= oph < sh and 0 <= opw < sw:
        return F.conv_transpose2d(gy.double(), w.double(), None, (sh, sw), (ph, pw), (oph, opw))
    xz = torch.zeros((gy.shape[0], w.shape[1], H, W), dtype=torch.float64, requires_grad=True)   # (stride 1 with rows no tap reaches)
    F.conv2d(xz, w.double(), None, (sh, sw), (ph, pw)).backward(gy.double())
    return xz.grad


def wgrad_ref(x, gy, kh, kw, stride, pad, x_abs=False):
    """Weight gradient by autograd in f64: -> [Cout,Cin,KH,KW]."""
    xd = x.double().abs() if x_abs else x.double()
    wz = torch.zeros((gy.shape[1], x.shape[1], kh, kw), dtype=torch.float64, requires_grad=True)
    F.conv2d(xd, wz, None, _pair(stride), _pair(pad)).backward(gy.double())
    return wz.grad


def cast(ref64, dtype):
    """The ONE rounding of an exact f64 reference to the kernel's output type."""
    if dtype in (torch.int32, torch.int64):
        assert torch.equal(ref64, ref64.round())
        return ref64.to(dtype)
    f32 = ref64.to(torch.float32)
    assert torch.equal(f32.double(), ref64), 'the reference is not exact in f32'      # (so f64 -> bf16 rounds once)
    return f32.to(dtype)


# --------------------------------------------------------------------------------------------- #
# GDN1 with a live gamma: y = t * (1 / (beta + gamma |t|))  (inverse: t * (beta + gamma |t|))
# --------------------------------------------------------------------------------------------- #
GAMMA_VALUES = (0.5, 1.0, 2.0)
GAMMA_DIAGONALS = 3


def live_gamma(C, g):
    """[C, C] with three random (cyclic) diagonals: every row and every column holds exactly three entries, each from {1/2, 1, 2}."""
    C = int(C)
    assert C >= GAMMA_DIAGONALS
    offs = torch.randperm(C, generator=g)[:GAMMA_DIAGONALS]
    vals = torch.tensor(GAMMA_VALUES)[torch.randint(0, len(GAMMA_VALUES), (GAMMA_DIAGONALS, C), generator=g)]
    gamma = torch.zeros(C, C)
    rows = torch.arange(C)
    for d in range(GAMMA_DIAGONALS):
        gamma[rows, (rows + int(offs[d])) % C] = vals[d]
    assert bool(((gamma != 0).sum(0) == GAMMA_DIAGONALS).all()) and bool(((gamma != 0).sum(1) == GAMMA_DIAGONALS).all())
    return gamma


def gdn_params(kind, C, g, inverse, tmax=None):
    """(gamma [C, C], beta [C], label) variants of one GDN1: the SAME three kinds of variant for both directions and both operand sets
    (`kind` is only validated and `inverse` is not used: they are taken so that a call names its case, and the values differ from case
    to case through the generator `g` alone).  gamma = 0: beta 1 -> the conv itself,
    beta 2 -> exactly half / double.  'live gamma': `live_gamma` and beta in {1, 2, 3} -- the norm is then a multiple of 1/2, a sum of
    non-negative terms, and (tmax given: asserted here; always asserted by gdn_restate) stays under EXACT_LIMIT quanta of 1/2: exact
    in f32 in any summation order."""
    assert kind in ('wide', 'narrow')
    out = [(torch.zeros(C, C), torch.ones(C), 'gamma 0 beta 1'), (torch.zeros(C, C), torch.full((C,), 2.0), 'gamma 0 beta 2')]
    gamma = live_gamma(C, g)
    beta = torch.randint(1, 4, (int(C),), generator=g).float()
    if tmax is not None:
        assert 2 * (3 + GAMMA_DIAGONALS * max(GAMMA_VALUES) * float(tmax)) < EXACT_LIMIT
    out.append((gamma, beta, 'live gamma'))
    return out


def _in_precision(t64, dtype):
    """The exact f64 conv output as the f32 tensor a kernel holds it in: the f32 accumulator, or that rounded once to bf16."""
    assert dtype in (torch.float32, torch.bfloat16)
    f32 = t64.to(torch.float32)
    assert torch.equal(f32.double(), t64), 't is not exact in f32'
    return f32 if dtype == torch.float32 else f32.to(torch.bfloat16).float()


def gdn_norm(t64, gamma, beta, t_gemm):
    """n = beta + gamma |cast(t, t_gemm)| (NCHW), computed in f64 and asserted to be an exact f32 number below EXACT_LIMIT quanta
    of 1/2 (every term is non-negative, so n is the sum of magnitudes: any partial sum in any order is exact as well) -> f32."""
    assert bool((gamma >= 0).all()) and bool((beta > 0).all())
    assert torch.equal(gamma * 2, (gamma * 2).round()) and torch.equal(beta * 2, (beta * 2).round())
    a = _in_precision(t64, t_gemm).double().abs()
    n64 = torch.einsum('oc,nchw->nohw', gamma.double(), a) + beta.double().view(1, -1, 1, 1)
    assert torch.equal(n64 * 2, (n64 * 2).round())
    assert float(n64.max()) * 2 < EXACT_LIMIT, 'norm of {} half quanta >= 2^24'.format(float(n64.max()) * 2)
    n32 = n64.to(torch.float32)
    assert torch.equal(n32.double(), n64)
    return n32


def gdn_restate(t64, gamma, beta, inverse, t_gemm, t_prod, out_dtype):
    """A kernel's documented GDN1 arithmetic in torch float32 on the CPU (IEEE, no fused operations), NCHW:
        n = beta + gamma |cast(t, t_gemm)|                  (exact, see gdn_norm)
        forward: r = f32(1) / n (correctly rounded), y = f32(cast(t, t_prod)) * r;      inverse: y = f32(cast(t, t_prod)) * n
    then ONE cast to out_dtype.  t_gemm / t_prod: torch.float32 (the accumulator) or torch.bfloat16 (the accumulator rounded once)."""
    n = gdn_norm(t64, gamma, beta, t_gemm)
    tp = _in_precision(t64, t_prod)
    y = tp * n if inverse else tp * (torch.ones((), dtype=torch.float32) / n)
    assert y.dtype == torch.float32
    return y.to(out_dtype)


def gdn_admissible(t64, gamma, beta, t_gemm, t_prod, out_dtype=torch.bfloat16):
    """The forward GDN1 of a kernel whose reciprocal is the hardware's (v_rcp_f32: within 1 ulp of 1 / n, so one of the correctly
    rounded r and its two f32 neighbours): -> ([cast(t * r') for r' in (r, below, above)], mask of the elements where these differ)."""
    n = gdn_norm(t64, gamma, beta, t_gemm)
    tp = _in_precision(t64, t_prod)
    r = torch.ones((), dtype=torch.float32) / n
    zero, inf = torch.zeros_like(r), torch.full_like(r, float('inf'))
    cands = [(tp * rr).to(out_dtype) for rr in (r, torch.nextafter(r, zero), torch.nextafter(r, inf))]
    many = (cands[1] != cands[0]) | (cands[2] != cands[0])
    return cands, many


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------------------------- #
# comparison
# --------------------------------------------------------------------------------------------- #
def _span(name, idx, group=1):
    v = torch.unique(idx // group)
    label = name if group == 1 else '{}//{}'.format(name, group)
    if v.numel() == 1:
        return '{} = {}'.format(label, int(v[0])), True
    return '{} in {}..{} ({} distinct)'.format(label, int(v.min()), int(v.max()), v.numel()), False


def assert_bits_equal(got, ref, what, layout='nhwc'):
    """torch.equal, and on failure: the number of mismatches, the first mismatching (n, oh, ow, c) with got / want there, and which
    index sets the mismatches span (one output row, a column range, one channel quad, one image, ...).
    layout: 'nhwc' / 'nchw' for 4-D outputs (both tensors in that layout); other ranks are reported by dimension number."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, '{}: shape {} != {}'.format(what, tuple(got.shape), tuple(ref.shape))
    assert got.dtype == ref.dtype, '{}: dtype {} != {}'.format(what, got.dtype, ref.dtype)
    if torch.equal(got, ref):
        return
    if got.dim() == 4:
        if layout == 'nchw':
            got, ref = got.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1)
        names = ('n', 'oh', 'ow', 'c')
    else:
        names = tuple('d{}'.format(i) for i in range(got.dim()))
    gd, rd = got.double(), ref.double()
    bad = (gd != rd) | (torch.isnan(gd) != torch.isnan(rd))
    idx = bad.nonzero()
    first = tuple(int(v) for v in idx[0])
    lines = ['{}: {} of {} elements differ'.format(what, idx.shape[0], bad.numel()),
             'first at ({}) = {}: got {!r}, want {!r}'.format(', '.join(names), first, got[first].item(), ref[first].item()),
             '{} NaN in the output'.format(int(torch.isnan(gd).sum()))]
    single = {}
    for d, name in enumerate(names):
        text, one = _span(name, idx[:, d])
        single[name] = one
        lines.append(text)
    if got.dim() == 4:
        lines.append(_span('c', idx[:, 3], 4)[0] + ' (channel quads)')
        flat_row = idx[:, 0] * got.shape[1] + idx[:, 1]
        lines.append('flat pixel m in {}..{}'.format(int(((flat_row * got.shape[2]) + idx[:, 2]).min()),
                                                    int(((flat_row * got.shape[2]) + idx[:, 2]).max())))
        if single['n'] and single['oh']:
            lines.append('=> all in ONE output row')
        elif single['n']:
            lines.append('=> all in ONE image')
    raise AssertionError('\n  '.join(lines))


def assert_bits_in(got, candidates, what, layout='nhwc'):
    """Every element of `got` equals that element of at least ONE of `candidates` (same shape and dtype each; NaN equals nothing);
    on failure: the number of elements that match no candidate and the first such coordinate with got / the candidates there."""
    got = got.detach().cpu()
    cands = [c.detach().cpu() for c in candidates]
    assert cands, '{}: no candidates'.format(what)
    for c in cands:
        assert got.shape == c.shape, '{}: shape {} != {}'.format(what, tuple(got.shape), tuple(c.shape))
        assert got.dtype == c.dtype, '{}: dtype {} != {}'.format(what, got.dtype, c.dtype)
    ok = torch.zeros(got.shape, dtype=torch.bool)
    for c in cands:
        ok |= got == c
    if bool(ok.all()):
        return
    if got.dim() == 4 and layout == 'nchw':
        got, ok, cands = got.permute(0, 2, 3, 1), ok.permute(0, 2, 3, 1), [c.permute(0, 2, 3, 1) for c in cands]
    names = ('n', 'oh', 'ow', 'c') if got.dim() == 4 else tuple('d{}'.format(i) for i in range(got.dim()))
    idx = (~ok).nonzero()
    first = tuple(int(v) for v in idx[0])
    raise AssertionError('{}: {} of {} elements match none of the {} admissible values\n  first at ({}) = {}: got {!r}, admissible {}'.format(
        what, idx.shape[0], ok.numel(), len(cands), ', '.join(names), first, got[first].item(),
        sorted(set(c[first].item() for c in cands))))


# --------------------------------------------------------------------------------------------- #
# guard-band arenas
# --------------------------------------------------------------------------------------------- #
def _fill_value(dtype, fill):
    if fill is not None:
        return fill
    return float('nan') if dtype.is_floating_point else INT_SENTINEL[dtype]


def arena(t, fill=None, device=None):
    """A contiguous copy of `t` (on `device`, default t's) inside a larger buffer filled with NaN (integer types: a large
    sentinel): >= 64 KB of fill on each side, the view at a 256-byte aligned address.  -> the view; `bands_untouched(view)` checks
    the fill afterwards."""
    device = t.device if device is None else torch.device(device)
    src = t.detach().contiguous()
    esz = src.element_size()
    nbytes = src.numel() * esz
    body = (nbytes + ALIGN - 1) // ALIGN * ALIGN
    total = GUARD_BYTES + ALIGN + body + GUARD_BYTES
    raw = torch.empty((total,), dtype=torch.uint8, device=device)
    value = _fill_value(src.dtype, fill)
    raw.view(src.dtype).fill_(value)
    off = GUARD_BYTES + (-(raw.data_ptr() + GUARD_BYTES)) % ALIGN
    view = raw[off:off + nbytes].view(src.dtype).view(src.shape)
    view.copy_(src)
    view._arena = (raw, off, nbytes, value)
    return view


def arena_like(shape, dtype, device, fill=None):
    """An output arena: the view itself holds the fill too (an element the kernel leaves unwritten stays NaN / sentinel)."""
    value = _fill_value(dtype, fill)
    return arena(torch.full(tuple(shape), value, dtype=dtype), fill=fill, device=device)


def bands(view):
    """(low band, high band) of an arena view as integer bit patterns, and the fill's pattern."""
    raw, off, nbytes, value = view._arena
    bits = _BITS[view.element_size()]
    pattern = torch.full((1,), value, dtype=view.dtype).view(bits)[0].item()
    return raw[:off].view(bits), raw[off + nbytes:].view(bits), pattern


def bands_untouched(view):
    lo, hi, pattern = bands(view)
    return bool((lo == pattern).all().item()) and bool((hi == pattern).all().item())


def assert_bands_untouched(view, what):
    lo, hi, pattern = bands(view)
    nlo, nhi = int((lo != pattern).sum().item()), int((hi != pattern).sum().item())
    if nlo or nhi:
        where = []
        if nlo:
            where.append('{} elements BELOW the tensor (nearest {} elements before its start)'.format(
                nlo, lo.numel() - int((lo != pattern).nonzero().max().item())))
        if nhi:
            where.append('{} elements ABOVE the tensor (first {} elements past its end)'.format(
                nhi, int((hi != pattern).nonzero().min().item())))
        raise AssertionError('{}: guard band written: {}'.format(what, '; '.join(where)))
