"""TEST INFRASTRUCTURE ONLY: the operand sets of the F32 form of the context-model scan (sc2_ar_scan_f32), on top of
tests/ref_ar_scan.py (imported, not edited: the step, the bound and the two assertions are the bf16 form's).

(a) `random_case_f32`: ref_ar_scan.random_case with the Gaussian weights rounded to f32 ONLY.  Every non-zero weight carries bits
below bf16's eight (the one f32 in 65 536 that happens to be a bf16 number is moved by one f32 ulp), so a scan that rounds the
weights to bf16 computes another function: its gaussian params leave the running f32 bound by a factor of 10 to 950 on
SMALL_SHAPES, while an f32 evaluation stays at 0.0014 to 0.041 of it (tests/test_ar_scan_f32_ref_cpu.py).

(b) `lowbits_case(matrix)`, one per weight matrix: ONE weight of that matrix is 1 + 2^-16 and meets an input of exactly 65 536;
the additive term of the same layer (bc, p1, b2 or b3: the layer's bias) is -65 536, so the output is exactly 1 with the f32 weight and
exactly 0 with its bf16 rounding (1.0).  Single-entry selection matrices carry that value to the mean of channel 0.  Every sum
has at most two non-zero terms and every value is an exact f32 number, so the kernel must equal the float64 reference bit for
bit; y = k + 1/4 on channel 0, so the symbol is k - 1 with the f32 weight and k with the rounded one: they differ by exactly 1.
Channel 1 is the carrier: y = 65 536, mean 0, hence y_hat = 65 536 at every pixel (the input the 'wc' case needs from the pixel
to the left; in the first column, where that tap is the zero border, p1 = +65 536 holds the unit at 0 and the mean is 0 under
either weight)."""
import numpy as np

import ref_ar_scan as RA

BIG = 65536.0
LOW = 1.0 + 2.0 ** -16                   # an f32 number whose bf16 rounding is 1.0
MATRICES = ('wc', 'w1', 'w2', 'w3')
LOWBITS_SHAPE = (2, 8, 8, 2, 3, 2)       # M, C1p, C2p, H, W, B
# the one unit of each layer that carries the value: ctx[J] -> h1[A] -> h2[Bq] -> mean of channel 0
J, A, BQ = 3, 5, 2
LEFT_TAP = 11                            # (dy, dx) = (0, -1)


def f32_only(a):
    return RA.f32(a).astype(np.float64)


def not_bf16(w):
    """Elementwise: the value is not a bf16 number."""
    return RA.bf16_round(w) != np.asarray(w, dtype=np.float64)


def bf16_weights(weights, names=MATRICES):
    """The dict with the named matrices rounded to bf16 (what a scan with bf16 operands would read)."""
    return {k: (RA.bf16_round(v) if k in names else v) for k, v in weights.items()}


def random_case_f32(M, C1p, C2p, H, W, B, seed=0):
    """ref_ar_scan.random_case drawn from the same generator, its Gaussian weights rounded to f32 instead of bf16."""
    keep = RA.bf16_round
    RA.bf16_round = f32_only
    try:
        case = RA.random_case(M, C1p, C2p, H, W, B, seed=seed)
    finally:
        RA.bf16_round = keep
    for name in MATRICES:
        w = RA.f32(case['weights'][name])
        plain = (w != 0) & ~not_bf16(w)
        w[plain] = np.nextafter(w[plain], np.float32(np.inf))
        case['weights'][name] = w.astype(np.float64)
    return case


def lowbits_case(matrix):
    """-> dict(weights, p1, y, scale_table, scale_bound, shape, matrix, symbols, symbols_bf16): the stated symbols [B, H*W, M]
    with the f32 weights and with `matrix` rounded to bf16."""
    assert matrix in MATRICES
    M, C1p, C2p, H, W, B = LOWBITS_SHAPE
    w = {'wc': np.zeros((RA.N_TAPS * M, 2 * M)), 'bc': np.zeros(2 * M), 'w1': np.zeros((2 * M, C1p)), 'w2': np.zeros((C1p, C2p)),
         'b2': np.zeros(C2p), 'w3': np.zeros((C2p, 2 * M)), 'b3': np.zeros(2 * M)}
    p1 = np.zeros((B, H, W, C1p))
    w['b3'][:M] = 1.5                                    # the scales: one table row for every symbol
    hit = np.ones((H, W), dtype=bool)                    # the pixels whose mean of channel 0 is 1 (f32) / 0 (bf16)
    if matrix == 'wc':
        w['wc'][LEFT_TAP * M + 1, J] = LOW               # the carrier channel of the pixel to the left
        w['bc'][J] = -BIG
        w['w1'][J, A] = 1.0
        p1[:, :, 0, A] = BIG                             # first column: the tap is the zero border, ctx[J] = -65536
        hit[:, 0] = False
    elif matrix == 'w1':
        w['bc'][J] = BIG
        w['w1'][J, A] = LOW
        p1[..., A] = -BIG
    else:
        p1[..., A] = 1.0 if matrix == 'w3' else BIG
    if matrix == 'w2':
        w['w2'][A, BQ] = LOW
        w['b2'][BQ] = -BIG
    elif matrix == 'w3':
        w['b2'][BQ] = BIG
    else:
        w['w2'][A, BQ] = 1.0
    if matrix == 'w3':
        w['w3'][BQ, M] = LOW
        w['b3'][M] = -BIG
    else:
        w['w3'][BQ, M] = 1.0
    rng = np.random.default_rng([7, MATRICES.index(matrix)])
    k = rng.integers(-40, 41, size=(B, H, W)).astype(np.float64)
    y = np.zeros((B, M, H, W))
    y[:, 0] = k + 0.25
    y[:, 1] = BIG
    sym = np.zeros((B, H, W, M), dtype=np.int32)
    sym[..., 0] = k
    sym[..., 1] = int(BIG)
    sym32 = sym.copy()
    sym32[..., 0] -= hit[None].astype(np.int32)
    for a in list(w.values()) + [p1, y]:
        assert np.array_equal(f32_only(a), a)
    assert int(not_bf16(w[matrix]).sum()) == 1 and not any(not_bf16(w[n]).any() for n in MATRICES if n != matrix)
    return {'weights': w, 'p1': p1, 'y': y, 'scale_table': RA.f32(RA.EXACT_TABLE), 'scale_bound': RA.EXACT_BOUND,
            'shape': LOWBITS_SHAPE, 'matrix': matrix, 'symbols': sym32.reshape(B, H * W, M),
            'symbols_bf16': sym.reshape(B, H * W, M)}


_CACHE = {}


def cached(kind, key):
    """(case, float64 scan_ref of it), computed once per process: kind 'random_f32' (key: a shape) or 'lowbits' (key: a matrix
    name).  Read-only."""
    k = (kind, tuple(key) if kind == 'random_f32' else key)
    if k not in _CACHE:
        case = random_case_f32(*key) if kind == 'random_f32' else lowbits_case(key)
        _CACHE[k] = (case, RA.scan_ref(case['weights'], case['p1'], case['y'], case['scale_table'], case['scale_bound']))
    return _CACHE[k]
