"""TEST INFRASTRUCTURE ONLY: a sequential numpy float64 reference of the context-model scan (csrc/ar_context.hip, the step
written in include/sc2_bottleneck.h above sc2_ar_scan_args) and the two operand sets its kernel-level tests run on.

`scan_ref` walks the pixels in raster order; `teacher_forced_ref` recomputes every pixel's gaussian params from a FINAL
y_hat_pad (at pixel p the causal taps touch only earlier pixels, whose values in that map are final) and carries a derived
bound on what an f32 evaluation in any summation order may differ by.

Weights are a dict of float64 arrays in the kernel's k-major packing: wc [12M, 2M] (k = tap * M + channel, the 12 causal taps of
the 5x5 type-A mask in raster order), bc [2M], w1 [2M, C1p], w2 [C1p, C2p], b2 [C2p], w3 [C2p, 2M], b3 [2M]; p1 [B, H, W, C1p];
y [B, M, H, W]; y_hat_pad [B, H + 2, W + 4, M] (two rows of border above, two columns on either side).

Exact set (the idiom of exact_ints.py): every value is a multiple of 1/8 and every sum of magnitudes times 8 stays below 2^24, so
every partial sum is an exact f32 number in any order and the kernel must equal the reference bit for bit.  Random set: Gaussian
bf16 weights, both LeakyReLU branches, held to the running bound."""
import math

import numpy as np

TAPS = [(-2, dx) for dx in range(-2, 3)] + [(-1, dx) for dx in range(-2, 3)] + [(0, -2), (0, -1)]
N_TAPS = 12
K_SPLIT = 4                              # the kernel's fixed k ranges per GEMV output (only the 'drop_k' mutant needs it)
SLOPE = float(np.float32(0.01))
U = 2.0 ** -24                           # unit roundoff of f32
EXACT_LIMIT = 1 << 24
EXACT_TABLE = [0.11, 0.25, 0.5] + [float(1 << i) for i in range(13)]      # ..., 4096
EXACT_BOUND = 0.11
FORCED_ENTRY = 4.0                       # a table entry: the `<=` boundary of the search
FORCED_NEGATIVE = -3.0
MUTANTS = ('tap_col', 'tap_rows', 'drop_k', 'p1_neighbour', 'slope0', 'lt', 'half_away', 'w2_pitch')

# (M, C1p, C2p, H, W, B): the kernel-level cases (tests/test_gpu_ar_scan.py); the first five also run on the random set
SMALL_SHAPES = [(6, 16, 16, 4, 5, 2), (5, 8, 24, 3, 7, 2), (3, 8, 8, 1, 9, 2), (7, 24, 16, 6, 1, 2), (24, 80, 64, 5, 6, 3)]
WIDE_SHAPES = [(136, 40, 48, 2, 3, 2), (264, 880, 704, 2, 3, 1), (512, 1280, 1280, 2, 2, 1)]
MANY_IMAGES = (4, 8, 8, 2, 3, 300)       # image i repeats image i mod 3
MANY_DISTINCT = 3
# A CHOSEN SEED.  With M = 4 three of the four scale channels are forced, so 18 scales of one free channel (about half of them
# negative: index 0) have to reach four more table rows for the six distinct indexes the preconditions demand; b3 is one value
# per channel and the ranges of y and p1 are fixed, so no operand can spread them by construction.  Seeds 0, 2 and 4 of 0..11
# fall short, 3 gives six rows.  check_exact_preconditions asserts it on the reference alone, so a change of the builder that
# loses the spread fails on the CPU, before any kernel is compared.
EXACT_SEEDS = {MANY_IMAGES[:5] + (MANY_DISTINCT,): 3}


def f32(a):
    return np.asarray(a, dtype=np.float32)


def bf16_round(a):
    """float -> the nearest bf16 value (ties to even), returned as float64.  Finite inputs only."""
    bits = f32(a).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


# --------------------------------------------------------------------------------------------- #
# the step
# --------------------------------------------------------------------------------------------- #
def _leaky(v, slope):
    return np.where(v < 0, slope * v, v)


def _drop(x, K):
    """The 'drop_k' mutant: the last k of the second of the kernel's four contiguous k ranges never reaches the sum."""
    kc = (K + K_SPLIT - 1) // K_SPLIT
    last = min(K, 2 * kc) - 1
    if last < kc:
        return x
    x = x.copy()
    x[..., last] = 0
    return x


def _repitch(w, pitch):
    """The 'w2_pitch' mutant: element (k, n) read at k * pitch + n of the same buffer."""
    K, N = w.shape
    flat = w.reshape(-1)
    return flat[(np.arange(K)[:, None] * pitch + np.arange(N)[None, :])]


def table_search(scales, scale_table, scale_bound, strict=False):
    """gc_symbols_indexes' search on max(scale, scale_bound), all in f32: n - 1 - #{t < n - 1 : s <= tab[t]}."""
    tab = f32(scale_table)
    s = np.maximum(f32(scales), np.float32(scale_bound))
    cmp = (s[..., None] < tab[:-1]) if strict else (s[..., None] <= tab[:-1])
    return (len(tab) - 1 - cmp.sum(-1)).astype(np.int32)


def quantise(y, means, half_away=False):
    """-> (symbol = rint(f32(y) - f32(mean)) in f32, ties to even; y_hat = f32(symbol + mean))."""
    m = f32(means)
    d = f32(y) - m
    q = np.sign(d) * np.floor(np.abs(d) + np.float32(0.5)) if half_away else np.rint(d)
    return q.astype(np.int32), (q.astype(np.float32) + m).astype(np.float32)


def scan_ref(weights, p1, y, scale_table, scale_bound, pix=None, y_hat_pad=None, mutant=None, dtype=np.float64):
    """The scan over pixels pix = (pix0, pix1) (default: all) in raster order, the batch vectorised.

    -> dict(symbols i32 [B, H*W*M], indexes i32 [B, H*W*M] (pixel-major, channel-minor), gaussian_params [B, H*W, 2M],
    y_hat_pad [B, H+2, W+4, M] float64 holding f32 values).  Pixels outside `pix` keep zeros in symbols / indexes /
    gaussian_params; `y_hat_pad` (default zeros) is copied, not written.  `mutant`: one of MUTANTS, a deliberately wrong step
    for the tests of the tests.  `dtype=np.float32` evaluates the four GEMVs in f32 (numpy's order), for checking the bound."""
    assert mutant is None or mutant in MUTANTS, mutant
    w = {k: np.asarray(v, dtype=dtype) for k, v in weights.items()}
    p1 = np.asarray(p1, dtype=dtype)
    B, H, W, C1p = p1.shape
    M = w['bc'].shape[0] // 2
    C2p = w['w2'].shape[1]
    assert w['wc'].shape == (N_TAPS * M, 2 * M) and w['w1'].shape == (2 * M, C1p) and w['w3'].shape == (C2p, 2 * M)
    assert tuple(np.shape(y)) == (B, M, H, W)
    pad = np.zeros((B, H + 2, W + 4, M)) if y_hat_pad is None else np.array(y_hat_pad, dtype=np.float64)
    assert pad.shape == (B, H + 2, W + 4, M)
    taps = list(TAPS)
    if mutant == 'tap_col':
        taps[11] = (0, -2)                                        # the pixel to the left read one column further left
    if mutant == 'tap_rows':
        taps = taps[5:10] + taps[0:5] + taps[10:]
    w2 = _repitch(w['w2'], C2p - 8) if mutant == 'w2_pitch' else w['w2']
    slope = 0.0 if mutant == 'slope0' else SLOPE
    drop = (lambda x: _drop(x, x.shape[-1])) if mutant == 'drop_k' else (lambda x: x)
    sym = np.zeros((B, H * W, M), dtype=np.int32)
    idx = np.zeros((B, H * W, M), dtype=np.int32)
    gps = np.zeros((B, H * W, 2 * M), dtype=np.float64)
    pix0, pix1 = (0, H * W) if pix is None else pix
    for p in range(pix0, pix1):
        h, x = divmod(p, W)
        xin = np.concatenate([pad[:, h + 2 + dy, x + 2 + dx, :] for dy, dx in taps], axis=1).astype(dtype)
        ctx = drop(xin) @ w['wc'] + w['bc']
        q = p if mutant != 'p1_neighbour' else (p + 1 if p + 1 < H * W else p - 1)
        h1 = _leaky(drop(ctx) @ w['w1'] + p1.reshape(B, H * W, C1p)[:, q], slope).astype(dtype)
        h2 = _leaky(drop(h1) @ w2 + w['b2'], slope).astype(dtype)
        gp = (drop(h2) @ w['w3'] + w['b3']).astype(np.float64)
        gps[:, p] = gp
        idx[:, p] = table_search(gp[:, :M], scale_table, scale_bound, strict=mutant == 'lt')
        sym[:, p], y_hat = quantise(np.asarray(y)[:, :, h, x], gp[:, M:], half_away=mutant == 'half_away')
        pad[:, h + 2, x + 2, :] = y_hat
    return {'symbols': sym.reshape(B, -1), 'indexes': idx.reshape(B, -1), 'gaussian_params': gps, 'y_hat_pad': pad}


# --------------------------------------------------------------------------------------------- #
# teacher forcing and the running bound
# --------------------------------------------------------------------------------------------- #
def gather_taps(y_hat_pad):
    """[B, H+2, W+4, M] -> [B, H*W, 12M]: every pixel's causal taps, k = tap * M + channel."""
    pad = np.asarray(y_hat_pad, dtype=np.float64)
    B, Hp, Wp, M = pad.shape
    H, W = Hp - 2, Wp - 4
    cols = [pad[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W, :] for dy, dx in TAPS]
    return np.concatenate(cols, axis=3).reshape(B, H * W, N_TAPS * M)


def _bounded_layer(x, bx, w, extra, leaky):
    """One layer in float64 with the bound of an f32 evaluation that sums the K products in any order and then adds the one
    additive term `extra` (the bias, or p1).  With u = 2^-24:
        bound[n] = (K + 2) u sum_k |in_k W_kn| + sum_k |W_kn| bound_in[k] + u |out[n]|
    A product passes through at most K + 1 roundings of the sum (the fmaf products are not rounded on their own), and
    (K + 1) u / (1 - (K + 1) u) <= (K + 2) u for every K below 4000, so the first term covers the summation to all orders; the
    second is the inputs' own error through the linear map; the third is the rounding of the one addition of the bias / p1, whose
    result is out.  LeakyReLU is 1-Lipschitz, so it passes the bound on; its negative branch multiplies in f32 and adds one more
    u |out| (also taken where the sign is within the bound of zero).
    -> (out, bound, sum of the magnitudes of ALL terms, the additive one included: the exactness precondition; pre-activation)."""
    K = w.shape[0]
    assert len(extra) == 1
    pre = x @ w + extra[0]
    products = np.abs(x) @ np.abs(w)
    mag = products + np.abs(extra[0])
    bound = (K + 2) * U * products + bx @ np.abs(w) + U * np.abs(pre)
    out = pre
    if leaky:
        out = _leaky(pre, SLOPE)
        bound = bound + U * np.abs(out) * ((pre < 0) | (np.abs(pre) <= bound))
    return out, bound, mag, pre


def teacher_forced_ref(weights, p1, y_hat_pad):
    """Every pixel's gaussian params in float64 from a final y_hat_pad, and the f32 bound on them.

    -> dict(gaussian_params [B, H*W, 2M], bound (same shape), h1_pre [B, H*W, C1p], h2_pre [B, H*W, C2p], mag_max: the largest
    sum of |terms| of any output of any layer).  The gathered taps are the kernel's own f32 values: their bound is 0."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    p1 = np.asarray(p1, dtype=np.float64)
    B, H, W, C1p = p1.shape
    xin = gather_taps(y_hat_pad)
    assert xin.shape[1] == H * W
    ctx, b, m0, _ = _bounded_layer(xin, np.zeros_like(xin), w['wc'], [w['bc']], False)
    h1, b, m1, pre1 = _bounded_layer(ctx, b, w['w1'], [p1.reshape(B, H * W, C1p)], True)
    h2, b, m2, pre2 = _bounded_layer(h1, b, w['w2'], [w['b2']], True)
    gp, b, m3, _ = _bounded_layer(h2, b, w['w3'], [w['b3']], False)
    return {'gaussian_params': gp, 'bound': b, 'h1_pre': pre1, 'h2_pre': pre2,
            'mag_max': max(float(m.max()) for m in (m0, m1, m2, m3))}


# --------------------------------------------------------------------------------------------- #
# operands
# --------------------------------------------------------------------------------------------- #
def real_widths(C1p, C2p):
    """The widths that carry weights; the columns / rows up to C1p / C2p are zero padding, as the model's packing leaves them."""
    return C1p - 3, C2p - 2


def _eighths(rng, lo, hi, shape):
    """Multiples of 1/8 in [lo, hi)."""
    return rng.integers(int(lo * 8), int(hi * 8), size=shape).astype(np.float64) / 8


def _pow2_above(v):
    return float(1 << int(math.ceil(math.log2(v + 1))))


def _sparse_signs(rng, rows, cols, cols_padded, fan_in):
    """[rows, cols_padded] with entries in {-1, 0, 1}: exactly `fan_in` non-zeros in each of the first `cols` columns, at least
    one in every row, zeros in the padding columns."""
    assert fan_in <= rows and fan_in * cols >= rows, (rows, cols, fan_in)
    used = [set() for _ in range(cols)]
    for i, r in enumerate(rng.permutation(rows)):
        used[i % cols].add(int(r))
    out = np.zeros((rows, cols_padded))
    for c in range(cols):
        more = rng.choice(rows, size=min(rows, fan_in + len(used[c])), replace=False)
        free = [int(r) for r in more if int(r) not in used[c]]
        picks = sorted(used[c]) + free[:fan_in - len(used[c])]
        out[picks, c] = rng.integers(0, 2, size=len(picks)) * 2 - 1
    return out


def exact_case(M, C1p, C2p, H, W, B, seed=0):
    """The exact operand set for one shape -> dict(weights, p1, y, scale_table, scale_bound, forced: {kind: scale channel},
    fan_in, shape).  Fan-ins: 8 for wc, 4 for w1 / w2, raised where fewer could not give every row a non-zero (w1 at
    2M = 272 rows over 37 columns).  The first min(3, M - 1) scale channels are forced through a zero w3 column: a table
    entry, scale_bound exactly, a negative value (with M = 3 the last is left to the free channel, whose scales take both
    signs)."""
    rng = np.random.default_rng([seed, M, C1p, C2p, H, W, B])
    C1, C2 = real_widths(C1p, C2p)
    fc = 8
    f1 = max(4, -(-2 * M // C1))
    f2 = max(4, -(-C1 // C2))
    wc = _sparse_signs(rng, N_TAPS * M, 2 * M, 2 * M, fc)
    w1 = _sparse_signs(rng, 2 * M, C1, C1p, f1)
    w2 = np.zeros((C1p, C2p))
    w2[:C1] = _sparse_signs(rng, C1, C2, C2p, f2)
    w3 = np.zeros((C2p, 2 * M))
    for n in range(2 * M):
        a, b = rng.choice(C2, size=2, replace=False)
        w3[a, n], w3[b, n] = 1.0, -1.0
    forced = dict(zip(('entry', 'bound', 'negative'), range(min(3, M - 1))))
    for ch in forced.values():
        w3[:, ch] = 0
    bc = _eighths(rng, -4, 4.125, 2 * M)
    # |y_hat| <= 32.5 (y_hat = y + (rint(d) - d)), so |ctx| <= 8 * 32.5 + 4; the offsets keep every pre-activation positive
    ctx_max = fc * 32.5 + 4
    c1 = _pow2_above(f1 * ctx_max)
    h1_max = c1 + 32 + f1 * ctx_max
    c2 = _pow2_above(f2 * h1_max)
    p1 = c1 + _eighths(rng, 0, 32, (B, H, W, C1p))
    b2 = c2 + _eighths(rng, 0, 32, C2p)
    b3 = _eighths(rng, -4, 4.125, 2 * M) - c1 * (w2[:C1].sum(0) @ w3)     # cancels the offsets: gp stays in the hundreds
    values = {'entry': FORCED_ENTRY, 'bound': float(np.float32(EXACT_BOUND)), 'negative': FORCED_NEGATIVE}
    for kind, ch in forced.items():
        b3[ch] = values[kind]
    y = _eighths(rng, -32, 32.125, (B, M, H, W))
    weights = {'wc': wc, 'bc': bc, 'w1': w1, 'w2': w2, 'b2': b2, 'w3': w3, 'b3': b3}
    return {'weights': weights, 'p1': p1, 'y': y, 'scale_table': f32(EXACT_TABLE), 'scale_bound': EXACT_BOUND,
            'forced': forced, 'fan_in': (fc, f1, f2), 'shape': (M, C1p, C2p, H, W, B)}


def check_exact_preconditions(case, ref):
    """Asserted on the reference alone: the sums are exact in f32, no pre-activation is negative, the rounding ties, the table
    rows and the forced scale cases are all there.  -> the figures."""
    M = case['shape'][0]
    w = case['weights']
    C1, C2 = real_widths(case['shape'][1], case['shape'][2])
    for name, fan in zip(('wc', 'w1', 'w2'), case['fan_in']):
        nz = w[name] != 0
        rows, cols = (C1, C2) if name == 'w2' else (nz.shape[0], C1 if name == 'w1' else nz.shape[1])
        assert set(np.unique(w[name])) <= {-1.0, 0.0, 1.0}
        assert (nz[:, :cols].sum(0) == fan).all() and not nz[:, cols:].any() and not nz[rows:].any(), name
        assert nz[:rows].any(1).all(), '{}: a row without a non-zero'.format(name)
    assert ((w['w3'] == 1).sum(0) == (w['w3'] == -1).sum(0)).all() and (np.abs(w['w3']).sum(0) <= 2).all()
    for a in list(w.values()) + [case['p1'], case['y']]:
        a = np.delete(a, list(case['forced'].values())) if a is w['b3'] else a
        assert np.array_equal(a * 8, np.round(a * 8)), 'operands must be multiples of 1/8'
    for name in ('wc', 'w1', 'w2', 'w3'):
        assert np.array_equal(bf16_round(w[name]), w[name])
    tf = teacher_forced_ref(w, case['p1'], ref['y_hat_pad'])
    assert np.array_equal(tf['gaussian_params'], ref['gaussian_params'])
    assert tf['mag_max'] * 8 < EXACT_LIMIT, 'sum |terms| * 8 = {} >= 2^24'.format(tf['mag_max'] * 8)
    pre_min = min(float(tf['h1_pre'].min()), float(tf['h2_pre'].min()))
    assert pre_min > 0, 'a pre-activation of {} takes the leaky branch'.format(pre_min)
    gp = ref['gaussian_params']
    d = f32(case['y']).transpose(0, 2, 3, 1).reshape(gp.shape[0], -1, M) - f32(gp[:, :, M:])
    ties = float((np.abs(d - np.floor(d)) == 0.5).mean())
    assert ties >= 0.02, 'only {:.1%} of the symbols are ties'.format(ties)
    n_idx = len(np.unique(ref['indexes']))
    assert n_idx >= 6, 'only {} distinct indexes'.format(n_idx)
    s = f32(gp[:, :, :M])
    assert (s == np.float32(FORCED_ENTRY)).any(), 'no scale equal to a table entry'
    assert (s == np.float32(case['scale_bound'])).any(), 'no scale equal to scale_bound'
    assert (s < 0).any(), 'no negative scale'
    for kind, ch in case['forced'].items():
        want = {'entry': FORCED_ENTRY, 'bound': np.float32(EXACT_BOUND), 'negative': FORCED_NEGATIVE}[kind]
        assert (s[:, :, ch] == np.float32(want)).all(), kind
    return {'mag_max_x8': tf['mag_max'] * 8, 'pre_min': pre_min, 'ties': ties, 'distinct_indexes': n_idx}


def random_case(M, C1p, C2p, H, W, B, seed=0):
    """The random operand set: Gaussian weights scaled by 1 / sqrt(fan_in) and rounded to bf16 (zero padding kept), p1 and the
    biases centred on 0 so that both LeakyReLU branches occur, y ~ 8 N(0, 1), GaussianConditional's default scale table."""
    rng = np.random.default_rng([seed + 1000, M, C1p, C2p, H, W, B])
    C1, C2 = real_widths(C1p, C2p)

    def gauss(rows, cols, rows_p, cols_p):
        out = np.zeros((rows_p, cols_p))
        out[:rows, :cols] = bf16_round(rng.standard_normal((rows, cols)) / math.sqrt(rows))
        return out

    def vec(n, std):
        return f32(rng.standard_normal(n) * std).astype(np.float64)
    weights = {'wc': gauss(N_TAPS * M, 2 * M, N_TAPS * M, 2 * M), 'bc': vec(2 * M, 1.0),
               'w1': gauss(2 * M, C1, 2 * M, C1p), 'w2': gauss(C1, C2, C1p, C2p), 'b2': vec(C2p, 1.0),
               'w3': gauss(C2, 2 * M, C2p, 2 * M), 'b3': vec(2 * M, 1.0)}
    table = np.exp(np.linspace(math.log(0.11), math.log(256), 64)).astype(np.float32)
    return {'weights': weights, 'p1': vec((B, H, W, C1p), 4.0), 'y': vec((B, M, H, W), 8.0), 'scale_table': table,
            'scale_bound': 0.11, 'shape': (M, C1p, C2p, H, W, B)}


def check_random_preconditions(case, ref):
    """At least 20 % of h1 and of h2 (the columns that carry weights) fall on each LeakyReLU branch.  -> the shares."""
    C1, C2 = real_widths(case['shape'][1], case['shape'][2])
    tf = teacher_forced_ref(case['weights'], case['p1'], ref['y_hat_pad'])
    out = {}
    for name, pre in (('h1', tf['h1_pre'][..., :C1]), ('h2', tf['h2_pre'][..., :C2])):
        neg = float((pre < 0).mean())
        assert 0.2 <= neg <= 0.8, '{}: {:.1%} of the pre-activations are negative'.format(name, neg)
        out[name + '_negative'] = neg
    return out


def bound_ratio(gp, tf):
    """The largest |gp - float64 value| / bound (0 / 0 counts as 0: a value the bound pins exactly and that is met)."""
    err = np.abs(np.asarray(gp, dtype=np.float64) - tf['gaussian_params'])
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / tf['bound'])
    return float(np.max(r))


_CACHE = {}


def cached(kind, shape, seed=None):
    """(case, scan_ref of it) computed once per process and shared: treat both as read-only."""
    seed = EXACT_SEEDS.get(tuple(shape), 0) if seed is None else seed
    key = (kind, tuple(shape), seed)
    if key not in _CACHE:
        case = (exact_case if kind == 'exact' else random_case)(*shape, seed=seed)
        ref = scan_ref(case['weights'], case['p1'], case['y'], case['scale_table'], case['scale_bound'])
        _CACHE[key] = (case, ref)
    return _CACHE[key]


# --------------------------------------------------------------------------------------------- #
# the two assertions a scan is held to (the kernel on the GPU, the mutants on the CPU)
# --------------------------------------------------------------------------------------------- #
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_exact(got, ref):
    """Exact set: symbols, indexes, gaussian_params and y_hat_pad equal the reference bit for bit (the reference's float64
    values are exact f32 numbers there, so the one cast below rounds nothing)."""
    for name in ('gaussian_params', 'y_hat_pad'):
        r32 = f32(ref[name])
        assert np.array_equal(r32.astype(np.float64), ref[name]), 'the reference {} is not exact in f32'.format(name)
        g = f32(got[name])
        if not _same_bits(g, r32):
            bad = np.argwhere(g.view(np.uint32) != r32.view(np.uint32))
            first = tuple(int(v) for v in bad[0])
            raise AssertionError('{}: {} of {} elements differ, first at {}: got {!r}, want {!r}'.format(
                name, len(bad), g.size, first, float(g[first]), float(r32[first])))
    for name in ('symbols', 'indexes'):
        g, r = np.asarray(got[name], dtype=np.int32), np.asarray(ref[name], dtype=np.int32)
        if not _same_bits(g, r):
            bad = np.argwhere(g != r)
            first = tuple(int(v) for v in bad[0])
            raise AssertionError('{}: {} of {} elements differ, first at {}: got {}, want {}'.format(
                name, len(bad), g.size, first, int(g[first]), int(r[first])))


def assert_random(case, got):
    """Random set: gaussian_params within teacher_forced_ref's bound of the float64 value computed from the scan's OWN final
    y_hat_pad, elementwise; and, each given the scan's own gaussian_params, exactly: symbols = the f32 rint, indexes = the
    table search, y_hat_pad = f32(symbol + mean).  -> the largest |err| / bound."""
    M, _, _, H, W, _ = case['shape']
    gp = np.asarray(got['gaussian_params'], dtype=np.float64)
    B = gp.shape[0]
    tf = teacher_forced_ref(case['weights'], case['p1'], got['y_hat_pad'])
    err = np.abs(gp - tf['gaussian_params'])
    ratio = bound_ratio(gp, tf)
    over = ~(err <= tf['bound'])
    if over.any():
        first = tuple(int(v) for v in np.argwhere(over)[0])
        raise AssertionError('gaussian_params: {} of {} elements outside the bound (largest |err| / bound {:.3g}); first at '
                             '(image, pixel, channel) {}: got {!r}, float64 {!r}, bound {:.3g}'.format(
                                 int(over.sum()), over.size, ratio, first, gp[first], tf['gaussian_params'][first],
                                 tf['bound'][first]))
    y = np.asarray(case['y']).transpose(0, 2, 3, 1).reshape(B, H * W, M)
    sym, y_hat = quantise(y, gp[:, :, M:])
    assert np.array_equal(np.asarray(got['symbols']).reshape(B, H * W, M), sym), 'symbols != rint(y - mean) in f32'
    idx = table_search(gp[:, :, :M], case['scale_table'], case['scale_bound'])
    assert np.array_equal(np.asarray(got['indexes']).reshape(B, H * W, M), idx), 'indexes != the table search'
    inner = f32(np.asarray(got['y_hat_pad'])[:, 2:, 2:W + 2, :]).reshape(B, H * W, M)
    assert _same_bits(inner, y_hat), 'y_hat_pad != f32(symbol + mean)'
    return ratio
