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
