"""-m gpu: every convolution / GEMM entry of hip.py against the INTEGER convolution, zero mismatches allowed.

Method (tests/exact_ints.py): operands are small integers, so every product and every partial sum (< 2^24) is an exact f32 number in
any summation order, inside the MFMA's 32-term sum as well.  A correct kernel equals the f64 reference bit for bit; a bf16 store
equals `exact.to(bfloat16)`.  Two operand sets per case: 'wide' ({-3..3}: outputs in the hundreds, the bf16 store's rounding and its
ties are exercised) and 'narrow' ({-1, 0, 1}, K p^2 <= 1024, max|ref| <= 256 asserted: one missing term shows through a bf16 store).
Every operand a case hands to a wrapper sits in a NaN arena (>= 64 KB of NaN on both sides): a read past an operand poisons the
output.  Where a wrapper takes `out=`, the output sits in an arena too and its bands are asserted untouched.

There is no tolerance in this file: every comparison is torch.equal (through exact_ints.assert_bits_equal, which names the first
mismatching coordinate and the index sets the mismatches span), membership in a set of at most three exact values
(exact_ints.assert_bits_in: the two hardware-reciprocal kernels) or an integer equality.

Cases come from each family's `*_supported` predicate and tile constants:
  conv2d_fwd          128-pixel tiles (generic 32 / 48 / 64 / 96 / 128-row tiles), 256-pixel 8-wave tiles, K slabs of 32, ring of 2 - 4
  conv3x3_win         28 / 14 / 7 maps: 7 rows, one image, four images per tile; stride 2: 56 / 28 / 14
  conv1x1_win         208-pixel tiles;  conv1x1_stream 128 (K = 512: 64) pixel units;  conv1x1_kres 32 (K = 2048: 16) pixel units
  conv1x1_pair        112-pixel tiles;  conv2x2_win 4 rows x 55-column segments;  conv2x2_c48 16-pixel tiles;  fc 128-row tiles
  conv2d_wgrad        32-pixel slabs, 128-column tiles;  conv2d_f32 / split 128-pixel tiles, 32-pixel units of the persistent first stage

GDN1 with a live gamma (nothing is set aside): the forward form's division is not integer-closed, but it is two IEEE f32 operations
on exact operands.  gamma has three entries from {1/2, 1, 2} per row and column and beta is in {1, 2, 3}, so n = beta + gamma |t| is a
multiple of 1/2, exact in f32 in any summation order; r = 1.0f / n and y = t * r (inverse: y = t * n) then give the same bits on the CPU
as on the device, and exact_ints.gdn_restate IS that arithmetic in torch float32.  What differs between the kernel families -- whether
t enters the second GEMM, and the product, as the f32 accumulator or rounded to bf16 -- is the GDN_FAMILIES table below, each row
taken from the family's own comment.  Every fused-GDN test runs gamma = 0 (beta 1: the conv itself; beta 2: exactly half / double)
and the live gamma, forward and inverse, on both operand sets, f32 and bf16 outputs; conv0_gdn96 and conv2_gdn48, whose forward form
multiplies by the hardware reciprocal (within 1 ulp), must hit one of the bf16 values admissible under it (assert_bits_in) -- a
single value on the narrow set and on all but < 0.1 % of the wide set's elements.  tests/test_exact_ints_cpu.py proves on the
references alone, for exactly these cases, that the norms are exact, that t * (1 / n) and t / n differ on > 5 % of the f32
outputs (the order of operations is visible), how few elements are ambiguous, and that a dropped gamma entry, swapped gamma rows or
columns, a beta added behind the reciprocal and the other precision of |t| each change the expected bits.

Not in arenas: conv2d_dgrad packs its sub-filters and conv2d_wgrad / the wrappers without `out=` allocate their outputs inside the
wrapper, so those packed weights and outputs are ordinary allocations; x, dY and the weight given to the wrapper are in arenas.
conv2d_wgrad's 128-channel A/B form is selected with hip.configure(wgrad_ct=128): the policy field has no SC2_* variable in
tools/env_policy.py, so monkeypatch.setenv cannot reach it; the test puts the default back itself.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import exact_ints as E  # noqa: E402

KINDS = ['wide', 'narrow']
BF16 = torch.bfloat16


# --------------------------------------------------------------------------------------------- #
# plumbing
# --------------------------------------------------------------------------------------------- #
def A(t, dev):
    """Any operand -> its NaN arena on the device."""
    return E.arena(t, device=dev)


def X(x_nchw, dev, dtype=BF16):
    """Integer NCHW activations -> NHWC `dtype` in an arena on the device."""
    return E.arena(E.nhwc(x_nchw).to(dtype), device=dev)


def operands(kind, cin, cout, k, H, W, N, seed=0):
    kh, kw = (k, k) if isinstance(k, int) else k
    K = cin * kh * kw
    g = E.gen(cin, cout, kh, kw, H, W, N, seed, kind == 'wide')
    x = E.operand(kind, (N, cin, H, W), K, g)
    w = E.operand(kind, (cout, cin, kh, kw), K, g)
    return g, K, x, w


def epilogue(conv64, bias=None, res=None, relu=False, mask=None):
    """The documented order in f64: acc + bias [+ residual] -> ReLU / ReLU-gradient mask; all NCHW."""
    y = conv64
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if relu:
        y = torch.relu(y)
    if mask is not None:
        y = torch.where(mask.double() > 0, y, torch.zeros_like(y))
    return y


def want_nhwc(ref64, dtype=BF16):
    return E.nhwc(E.cast(ref64, dtype))


def out_shape(S, fmt, N, cout, OH, OW):
    hip = S.hip
    if fmt == hip.OUT_BF16_NHWC:
        return (N, OH, OW, cout), BF16
    if fmt == hip.OUT_F32_NHWC:
        return (N, OH, OW, cout), torch.float32
    return (N, cout, OH, OW), torch.float32 if fmt == hip.OUT_F32_NCHW else torch.int32


def conv2d(S, dev, xd, wp, cout, k, stride, pad, ref64, what, fmt=None, restate=None, **kw):
    """One sc2_conv2d_fwd launch into an output arena, compared with the f64 reference (NCHW) cast once; bands checked.
    restate: a function of the output dtype that gives the wanted NCHW tensor itself (the GDN1 restatements, whose f32 operations
    round), ref64 then only carries the shape."""
    hip = S.hip
    fmt = hip.OUT_BF16_NHWC if fmt is None else fmt
    kh, kw_ = (k, k) if isinstance(k, int) else k
    N, cout_r, OH, OW = ref64.shape
    shape, dtype = out_shape(S, fmt, N, cout, OH, OW)
    out = E.arena_like(shape, dtype, dev)
    got = hip.conv2d_fwd(xd, wp, cout, kh, kw_, stride, pad, out_format=fmt, out=out, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    nchw = fmt in (hip.OUT_F32_NCHW, hip.OUT_I32_NCHW_SYM)
    want = E.cast(ref64, dtype) if restate is None else restate(dtype)
    assert want.dtype == dtype
    E.assert_bits_equal(got, want if nchw else E.nhwc(want), what, layout='nchw' if nchw else 'nhwc')
    E.assert_bands_untouched(out, what)
    return got


def k_orders(S, cin):
    hip = S.hip
    orders = [hip.K_TAP_MAJOR, hip.K_TAP_MAJOR | hip.K_B_TILE_MAJOR]
    if cin % 32 == 0:
        orders += [hip.K_SLAB_MAJOR, hip.K_SLAB_MAJOR | hip.K_B_TILE_MAJOR]
    return orders


# --------------------------------------------------------------------------------------------- #
# conv2d_fwd: the generic 128-pixel tiles of 32 / 48 / 64 / 96 / 128 rows
# --------------------------------------------------------------------------------------------- #
GENERIC = [
    # (cin, cout, k, stride, pad, H, W, N)
    (16, 40, 3, 1, 1, 7, 50, 3),       # 48-row tile; rows of 50 straddle the 128-pixel tiles, image borders at 350 / 700 inside tiles; K = 144: tail slab of 16
    (24, 64, 3, 2, 1, 15, 15, 3),      # 64-row tile, stride 2, K = 216 (tail slab of 24)
    (8, 96, 3, 1, 1, 1, 1, 5),         # 96-row tile, a 1 x 1 map: k > H with padding, odd N, M = 5
    (32, 136, 3, 1, 1, 9, 13, 3),      # 128-row tiles, Cout not a multiple of the tile, M = 351
    (64, 128, 1, 2, 0, 9, 9, 1),       # 1x1 stride 2, K = 64: two slabs, shorter than the ring of three
    (40, 72, 5, 2, 2, 11, 12, 1),      # 96-row tile with 24 padding rows, K = 1000 (tail slab of 8)
    (8, 8, 2, 1, 1, 3, 4, 1),          # the smallest channel counts, 32-row tile, K = 32: one slab
    (8, 24, 1, 1, 0, 1, 1, 1),         # one pixel, K = 8
    (96, 200, 1, 1, 0, 6, 43, 1),      # 256 packed rows, 200 used; M = 258: two pixels in the third tile
]
GENERIC += [(8, c, 1, 1, 0, 1, m, 1) for c in (24, 48, 64, 96, 128) for m in (127, 128, 129)]     # M = one tile, one less, one more


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,k,stride,pad,H,W,N', GENERIC)
def test_conv2d_generic_tiles(S, dev, kind, cin, cout, k, stride, pad, H, W, N):
    """All K orders and all output formats of one geometry equal the integer conv, hence each other; EPI_BIAS; symbols with
    medians that are multiples of 0.25 (rintf meets ties)."""
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, k, H, W, N)
    bias, med = E.bias_ints(cout, g), E.quarter_medians(cout, g)
    E.check_bound(K, x, w, bias)
    ref = E.conv_ref(x, w, stride, pad)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd = X(x, dev)
    tag = 'conv2d {}->{} k{} s{} p{} {}x{}x{} {}'.format(cin, cout, k, stride, pad, N, H, W, kind)
    for order in k_orders(S, cin):
        wp = A(hip.pack_conv_weight(w.to(dev), order), dev)
        for fmt in (hip.OUT_BF16_NHWC, hip.OUT_F32_NCHW, hip.OUT_F32_NHWC):
            conv2d(S, dev, xd, wp, cout, k, stride, pad, ref, '{} order {} fmt {}'.format(tag, order, fmt), fmt=fmt, k_order=order)
        conv2d(S, dev, xd, wp, cout, k, stride, pad, epilogue(ref, bias), tag + ' + bias order {}'.format(order),
               epilogue=hip.EPI_BIAS, ep_beta=A(bias, dev), k_order=order)
        if hip.weight_rows(cout) % 128 != 0:
            sym = torch.round(ref - med.double().view(1, -1, 1, 1))          # round half to even, as rintf
            conv2d(S, dev, xd, wp, cout, k, stride, pad, sym, tag + ' symbols order {}'.format(order), fmt=hip.OUT_I32_NCHW_SYM,
                   ep_beta=A(med, dev), k_order=order)


STATIC = [
    # the encoder / decoder geometries of the FP bottleneck at the 224 x 224 operating point (N = 1) and small maps at an odd N
    (96, 48, 5, 2, 2, 112, 112, 1), (96, 48, 5, 2, 2, 9, 14, 3),
    (48, 24, 2, 1, 0, 56, 56, 1), (48, 24, 2, 1, 0, 5, 4, 3),
    (24, 512, 2, 1, 1, 27, 27, 1), (24, 512, 2, 1, 1, 3, 5, 3),
    (512, 256, 2, 1, 0, 28, 28, 1), (512, 256, 2, 1, 0, 6, 9, 3),
    (256, 256, 2, 1, 1, 55, 55, 1), (256, 256, 2, 1, 1, 4, 7, 3),
    (96, 96, 1, 1, 0, 11, 12, 1), (48, 48, 1, 1, 0, 7, 19, 3), (512, 512, 1, 1, 0, 9, 15, 1), (256, 256, 1, 1, 0, 13, 10, 3),   # the GDN GEMM geometries
]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,k,stride,pad,H,W,N', STATIC)
def test_conv2d_static_geometries(S, dev, monkeypatch, kind, cin, cout, k, stride, pad, H, W, N):
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, k, H, W, N)
    res = E.residual_ints((N, cout, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1), g)
    bias = E.bias_ints(cout, g)
    E.check_bound(K, x, w, bias, res)
    ref = E.conv_ref(x, w, stride, pad)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd = X(x, dev)
    tag = 'static {}->{} k{} {}x{}x{} {}'.format(cin, cout, k, N, H, W, kind)
    for order in k_orders(S, cin):
        wp = A(hip.pack_conv_weight(w.to(dev), order), dev)
        conv2d(S, dev, xd, wp, cout, k, stride, pad, ref, tag + ' order {}'.format(order), k_order=order)
        conv2d(S, dev, xd, wp, cout, k, stride, pad, ref, tag + ' f32 order {}'.format(order), fmt=hip.OUT_F32_NHWC, k_order=order)
    wp = A(hip.pack_conv_weight(w.to(dev)), dev)
    rd = A(E.nhwc(res), dev)
    for no_epx in (False, True):      # the residual read in the output layout (Cx_* / Gx_*) and through the plain epilogue
        if no_epx:
            monkeypatch.setenv('SC2_CONV_NO_EPX', '1')
        conv2d(S, dev, xd, wp, cout, k, stride, pad, epilogue(ref, bias, res, relu=True), tag + ' + bias + residual + relu, no_epx {}'.format(no_epx),
               epilogue=hip.EPI_BIAS_ADD_RELU, ep_beta=A(bias, dev), ep_x=rd)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,k,stride,pad,H,W,N', [(16, 24, 3, 1, 1, 7, 50, 3), (16, 40, 3, 1, 1, 7, 50, 3), (24, 64, 3, 2, 1, 15, 15, 3),
                                                         (40, 72, 5, 2, 2, 11, 12, 1), (8, 96, 1, 1, 0, 1, 129, 1), (32, 136, 3, 1, 1, 9, 13, 3)])
def test_conv2d_residual_epilogue_generic_tiles(S, dev, monkeypatch, kind, cin, cout, k, stride, pad, H, W, N):
    """EPI_BIAS_ADD_RELU on the generic 32 / 48 / 64 / 96 / 128-row tiles: the residual prefetched in the output layout (Gx_*) and,
    with conv_no_epx, read by the plain epilogue -- the same bits."""
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, k, H, W, N, seed=5)
    ref = E.conv_ref(x, w, stride, pad)
    if kind == 'narrow':
        E.check_narrow(ref)
    res, bias = E.residual_ints(tuple(ref.shape), g), E.bias_ints(cout, g)
    E.check_bound(K, x, w, bias, res)
    xd, wp, rd, bd = X(x, dev), A(hip.pack_conv_weight(w.to(dev)), dev), X(res, dev), A(bias, dev)
    for no_epx in (False, True):
        if no_epx:
            monkeypatch.setenv('SC2_CONV_NO_EPX', '1')
        conv2d(S, dev, xd, wp, cout, k, stride, pad, epilogue(ref, bias, res, relu=True),
               'residual epilogue {}->{} k{} {}x{}x{} no_epx {} {}'.format(cin, cout, k, N, H, W, no_epx, kind),
               epilogue=hip.EPI_BIAS_ADD_RELU, ep_beta=bd, ep_x=rd)


def test_conv0_pixel_pairs_exact(S, dev):
    """3 -> 96, k5 s2 p2 on the pixel-pair view (C_conv0): the operating-point width and an odd batch of small maps."""
    hip = S.hip
    for kind in KINDS:
        for N, H, W in ((1, 224, 224), (3, 7, 10), (1, 1, 2)):
            g, K, x, w = operands(kind, 3, 96, 5, H, W, N)
            E.check_bound(K, x, w)
            ref = E.conv_ref(x, w, 2, 2)
            if kind == 'narrow':
                E.check_narrow(ref)
            x4 = torch.zeros(N, H, W, 4)
            x4[..., :3] = E.nhwc(x)
            xp = A(x4.to(BF16).view(N, H, W // 2, 8), dev)
            wp = A(hip.pack_conv0_weight_pairs(w.to(dev)), dev)
            for fmt in (hip.OUT_BF16_NHWC, hip.OUT_F32_NCHW):
                conv2d(S, dev, xp, wp, 96, (5, 3), (2, 1), (2, 1), ref, 'conv0 pairs {}x{}x{} {} fmt {}'.format(N, H, W, kind, fmt), fmt=fmt)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,k,pad,dil,H,W,N', [(32, 128, 3, 2, 2, 9, 11, 3), (16, 136, 3, 4, 4, 12, 10, 1), (64, 256, 3, 2, 2, 1, 1, 1),
                                                      (24, 128, 3, 4, 4, 5, 26, 1), (8, 128, 1, 0, 2, 1, 129, 1)])
def test_conv2d_dilated(S, dev, kind, cin, cout, k, pad, dil, H, W, N):
    """Gd_128: dilation 2 and 4, the taps that fall outside a map smaller than the filter's reach."""
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, k, H, W, N, seed=dil)
    bias = E.bias_ints(cout, g)
    E.check_bound(K, x, w, bias)
    ref = E.conv_ref(x, w, 1, pad, dil)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd = X(x, dev)
    for order in k_orders(S, cin):
        wp = A(hip.pack_conv_weight(w.to(dev), order), dev)
        conv2d(S, dev, xd, wp, cout, k, 1, pad, ref, 'dilated d{} order {} {}'.format(dil, order, kind), k_order=order, dilation=dil)
        conv2d(S, dev, xd, wp, cout, k, 1, pad, epilogue(ref, bias, relu=True), 'dilated d{} + bias + relu {}'.format(dil, kind),
               fmt=hip.OUT_F32_NCHW, k_order=order, dilation=dil, epilogue=hip.EPI_BIAS_RELU, ep_beta=A(bias, dev))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N,H,W', [(1, 112, 112), (3, 9, 14), (1, 1, 1), (2, 6, 128), (1, 20, 127)])
def test_conv2d_lds_patch_kernel(S, dev, kind, N, H, W):
    """K_B_FRAG_MAJOR: the LDS-patch kernel of the second encoder conv; OW = 64 is its widest row."""
    hip = S.hip
    g, K, x, w = operands(kind, 96, 48, 5, H, W, N)
    bias = E.bias_ints(48, g)
    E.check_bound(K, x, w, bias)
    ref = E.conv_ref(x, w, 2, 2)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd = X(x, dev)
    assert hip.conv_patch_supported(tuple(xd.shape), 48, 5, 5, 2, 2)
    order = hip.K_SLAB_MAJOR | hip.K_B_FRAG_MAJOR
    wp = A(hip.pack_conv_weight(w.to(dev), order), dev)
    conv2d(S, dev, xd, wp, 48, 5, 2, 2, ref, 'patch kernel {}x{}x{} {}'.format(N, H, W, kind), k_order=order)
    conv2d(S, dev, xd, wp, 48, 5, 2, 2, epilogue(ref, bias), 'patch kernel + bias {}'.format(kind), k_order=order,
           epilogue=hip.EPI_BIAS, ep_beta=A(bias, dev))


# --------------------------------------------------------------------------------------------- #
# the forced variants: every variant of one geometry gives the integer conv, hence the same bits
# --------------------------------------------------------------------------------------------- #
BIG = [
    (512, 256, 2, 1, 0, 9, 9, 5),      # dec.conv2 geometry: 320 pixels = one 256-pixel tile + 64
    (256, 256, 2, 1, 1, 15, 16, 1),    # dec.conv4 geometry: 16 x 17 = 272; rows of 17 straddle the tile edge
    (512, 256, 2, 1, 0, 17, 17, 1),    # M = 256: one tile exactly
    (256, 256, 2, 1, 1, 14, 16, 1),    # M = 255
    (256, 256, 2, 1, 1, 1, 256, 1),     # 2 x 257 = 514: two tiles + 2
    (64, 512, 1, 1, 0, 20, 20, 1),     # generic 256-wide, two n-tiles, K = 64: two slabs, shorter than the ring
    (24, 384, 3, 2, 1, 30, 30, 3),     # Cout 384: 128-wide 8-wave tiles, K = 216 (tail slab), odd N
    (32, 128, 3, 1, 1, 1, 1, 1),       # one pixel, k > H
    (40, 256, 1, 1, 0, 1, 257, 1),     # K = 40: a tail slab only after one whole slab; M = one tile + 1
]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,k,stride,pad,H,W,N', BIG)
def test_conv2d_forced_big_tile_variants(S, dev, monkeypatch, kind, cin, cout, k, stride, pad, H, W, N):
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, k, H, W, N)
    bias = E.bias_ints(cout, g)
    E.check_bound(K, x, w, bias)
    ref = E.conv_ref(x, w, stride, pad)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd = X(x, dev)
    packed = {o: A(hip.pack_conv_weight(w.to(dev), o), dev) for o in k_orders(S, cin)}
    # (half, big4, patch3, persist): '0', '1', 'r4', 'w2' as test_conv_big_tile sets them (conv_patch3 0 but for 'w2'), each with the
    # one-workgroup-per-tile form, then the persistent forms 1 .. 3 of the two decoder geometries
    variants = [('0', '0', '0', '0'), ('1', '0', '0', '0'), ('0', '1', '0', '0'), ('0', '0', '2', '0')]
    variants += [('0', '0', '0', p) for p in ('1', '2', '3')]
    for v in variants:
        monkeypatch.setenv('SC2_CONV_FORCE_BIG', '1')
        monkeypatch.setenv('SC2_CONV_HALF', v[0])
        monkeypatch.setenv('SC2_CONV_BIG4', v[1])
        monkeypatch.setenv('SC2_CONV_PATCH3', v[2])
        monkeypatch.setenv('SC2_CONV_PERSIST', v[3])
        tag = 'big tile {}->{} k{} {}x{}x{} {} variant {}'.format(cin, cout, k, N, H, W, kind, v)
        for o, wp in packed.items():
            conv2d(S, dev, xd, wp, cout, k, stride, pad, ref, tag + ' order {}'.format(o), k_order=o)
            conv2d(S, dev, xd, wp, cout, k, stride, pad, ref, tag + ' f32 nchw order {}'.format(o), fmt=hip.OUT_F32_NCHW, k_order=o)
        conv2d(S, dev, xd, packed[hip.K_TAP_MAJOR], cout, k, stride, pad, epilogue(ref, bias, relu=True), tag + ' + bias + relu',
               epilogue=hip.EPI_BIAS_RELU, ep_beta=A(bias, dev))
    monkeypatch.delenv('SC2_CONV_FORCE_BIG')
    monkeypatch.setenv('SC2_CONV_NO_BIG', '1')
    conv2d(S, dev, xd, packed[hip.K_TAP_MAJOR], cout, k, stride, pad, ref, 'no_big twin')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,H,W,N', [
    (64, 256, 14, 14, 3),      # a 256-pixel tile spans two images
    (32, 128, 7, 7, 11),       # five images per tile, a single channel slab, odd N
    (96, 384, 5, 31, 1),       # the widest row, three slabs, Cout 384
    (32, 256, 1, 1, 1),        # 1 x 1 map
    (64, 128, 16, 16, 1),      # M = 256 / 128 exactly
    (32, 128, 3, 43, 1),       # M = 129
])
def test_conv2d_3x3_window_variants(S, dev, monkeypatch, kind, cin, cout, H, W, N):
    """conv_patch3 1 / 256 (one staged window per slab, 128- / 256-wide tiles) and 0 (im2col gather): the same bits."""
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, 3, H, W, N)
    bias = E.bias_ints(cout, g)
    E.check_bound(K, x, w, bias)
    conv = E.conv_ref(x, w, 1, 1)
    if kind == 'narrow':
        E.check_narrow(conv)
    ref = epilogue(conv, bias, relu=True)
    xd = X(x, dev)
    order = hip.preferred_k_order(cin, 3, 3)
    assert order & hip.K_SLAB_MAJOR
    wp = A(hip.pack_conv_weight(w.to(dev), order), dev)
    bd = A(bias, dev)
    for flag in ('1', '256', '0'):
        monkeypatch.setenv('SC2_CONV_PATCH3', flag)
        conv2d(S, dev, xd, wp, cout, 3, 1, 1, ref, '3x3 window variant {} {}->{} {}x{}x{} {}'.format(flag, cin, cout, N, H, W, kind),
               epilogue=hip.EPI_BIAS_RELU, ep_beta=bd, k_order=order)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,H,W,N', [(128, 128, 56, 56, 1), (64, 256, 29, 27, 3), (32, 256, 1, 1, 1), (32, 128, 2, 255, 1),
                                            (32, 256, 31, 33, 1), (96, 256, 3, 513, 1)])
def test_conv2d_3x3_stride2_variants(S, dev, monkeypatch, kind, cin, cout, H, W, N):
    """conv_s2 128 / 256 (static-geometry 8-wave tiles, out-of-image taps sent out of range) and 0: the same bits; odd sizes,
    M = 128 / 256 +- 1 (2 x 255 -> 128; 31 x 33 -> 16 x 17 = 272; 3 x 513 -> 2 x 257 = 514)."""
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, 3, H, W, N)
    bias = E.bias_ints(cout, g)
    E.check_bound(K, x, w, bias)
    conv = E.conv_ref(x, w, 2, 1)
    if kind == 'narrow':
        E.check_narrow(conv)
    ref = epilogue(conv, bias, relu=True)
    xd = X(x, dev)
    bd = A(bias, dev)
    for order in (hip.preferred_k_order(cin, 3, 3), hip.K_TAP_MAJOR):
        wp = A(hip.pack_conv_weight(w.to(dev), order), dev)
        for flag in ('128', '256', '0'):
            monkeypatch.setenv('SC2_CONV_S2', flag)
            conv2d(S, dev, xd, wp, cout, 3, 2, 1, ref, '3x3 s2 variant {} order {} {}->{} {}x{}x{} {}'.format(flag, order, cin, cout, N, H, W, kind),
                   epilogue=hip.EPI_BIAS_RELU, ep_beta=bd, k_order=order)


# --------------------------------------------------------------------------------------------- #
# the natural dispatch boundary: big_tile_eligible crossed without a switch
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('kind', KINDS)
def test_conv2d_natural_big_tile_boundary(S, dev, kind):
    """Default policy, 1x1, K = 1024: Cout = 256 at M = 49 151 (128-pixel tiles), 49 152 and 49 153 (256-pixel 8-wave tiles: the
    threshold is M >= 256 * 192), and a Cout = 128 neighbour that must not take the big tile.  One reference for the largest M: a 1x1
    conv is per pixel, so the smaller launches see its first pixels."""
    hip = S.hip
    p = hip.get_policy()
    assert not p.conv_force_big and not p.conv_no_big
    M = 49153
    g, K, x, w = operands(kind, 1024, 256, 1, 1, M, 1)
    E.check_bound(K, x, w)
    ref = (w.reshape(256, 1024).double() @ x.reshape(1024, M).double()).reshape(1, 256, 1, M)
    assert torch.equal(ref[:, :, :, :300], E.conv_ref(x[:, :, :, :300], w))
    if kind == 'narrow':
        E.check_narrow(ref)
    wp = A(hip.pack_conv_weight(w.to(dev), hip.K_B_TILE_MAJOR), dev)
    wp128 = A(hip.pack_conv_weight(w[:128].to(dev), hip.K_B_TILE_MAJOR), dev)
    for m in (49151, 49152, 49153):
        xd = X(x[:, :, :, :m], dev)
        conv2d(S, dev, xd, wp, 256, 1, 1, 0, ref[:, :, :, :m], 'natural boundary M = {} Cout 256 {}'.format(m, kind), k_order=hip.K_B_TILE_MAJOR)
        conv2d(S, dev, xd, wp128, 128, 1, 1, 0, ref[:, :128, :, :m], 'natural boundary M = {} Cout 128 {}'.format(m, kind),
               k_order=hip.K_B_TILE_MAJOR)
        del xd


# --------------------------------------------------------------------------------------------- #
# data and weight gradients
# --------------------------------------------------------------------------------------------- #
DGRAD = [
    # (cin, cout, k, stride, pad, H, W, N)
    (16, 24, 3, 2, 1, 9, 10, 3),       # four parity classes, odd / even sizes
    (8, 16, 1, 2, 0, 7, 8, 1),         # 1x1 stride 2: three of four classes are reached by no tap (zero)
    (24, 8, 5, 2, 2, 12, 11, 1),       # k5 s2 p2: classes with 3 x 3, 3 x 2, 2 x 3, 2 x 2 taps
    (16, 16, 2, 2, 0, 8, 8, 2),        # k2 s2: one tap per class
    (8, 32, 3, 1, 1, 6, 7, 3),         # stride 1: the single class
    (256, 256, 2, 1, 1, 5, 6, 1),      # dec.conv4's gradient: the window-plane 2x2 kernel
    (512, 256, 2, 1, 0, 6, 5, 3),      # dec.conv2's gradient: two 256-channel halves of that kernel through out= / channel0
    (16, 8, 3, 2, 1, 1, 1, 1),         # 1 x 1 input
    (8, 8, 3, 3, 0, 10, 11, 1),        # stride 3: nine classes, one tap each
]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,k,stride,pad,H,W,N', DGRAD)
def test_conv2d_dgrad_exact(S, dev, kind, cin, cout, k, stride, pad, H, W, N):
    hip = S.hip
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g, K, gy, w = operands(kind, cout, cin, k, OH, OW, N)         # (the gradient's K: Cout x taps)
    w = w.permute(1, 0, 2, 3).contiguous()                          # [Cout, Cin, k, k]
    E.check_bound(K, gy, w)
    ref = E.dgrad_ref(gy, w, stride, pad, (H, W))
    if kind == 'narrow':
        E.check_narrow(ref)
    gyd = X(gy, dev)
    wd = A(w, dev)
    for dt in (BF16, torch.float32):
        got = hip.conv2d_dgrad(gyd, wd, stride, pad, (H, W), out_dtype=dt)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, want_nhwc(ref, dt), 'dgrad {}->{} k{} s{} p{} {}x{}x{} {} {}'.format(cin, cout, k, stride, pad, N, H, W, dt, kind))


WGRAD = [
    # (cin, cout, k, stride, pad, H, W, N)            K of the gradient GEMM = N OH OW
    (64, 64, 1, 1, 0, 56, 56, 3),      # 9 408 pixels
    (8, 96, 3, 1, 1, 6, 6, 1),         # 36 pixels: one whole slab + 4
    (16, 24, 3, 2, 1, 9, 10, 3),
    (24, 8, 5, 2, 2, 12, 11, 1),
    (128, 256, 1, 1, 0, 1, 31, 1),     # one slab less one pixel; the 256-channel tile form
    (8, 8, 1, 1, 0, 1, 32, 1), (8, 8, 1, 1, 0, 1, 33, 1),      # one slab, one more
    (256, 136, 1, 1, 0, 5, 5, 1),      # Cout not a tile multiple
    (8, 16, 3, 1, 1, 1, 1, 5),         # 1 x 1 maps
    (40, 48, 2, 1, 0, 7, 7, 2),        # 160 k-columns: a second, partial 128-column tile
]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('x_abs', [False, True])
@pytest.mark.parametrize('cin,cout,k,stride,pad,H,W,N', WGRAD)
def test_conv2d_wgrad_exact(S, dev, kind, x_abs, cin, cout, k, stride, pad, H, W, N):
    hip = S.hip
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    Kg = N * OH * OW
    g = E.gen(cin, cout, k, H, W, N, kind == 'wide')
    x = E.operand(kind, (N, cin, H, W), Kg, g)
    gy = E.operand(kind, (N, cout, OH, OW), Kg, g)
    E.check_bound(Kg, x, gy)
    ref = E.wgrad_ref(x, gy, k, k, stride, pad, x_abs=x_abs)
    if kind == 'narrow':
        E.check_narrow(ref)
    for ct in (0, 128) if cout > 128 else (0,):      # (more than 128 channels: the 256-channel tile, and its 128-channel A/B form)
        hip.configure(wgrad_ct=ct)
        try:
            got = hip.conv2d_wgrad(X(x, dev), X(gy, dev), k, k, stride, pad, x_abs=x_abs)
            torch.cuda.synchronize()
        finally:
            hip.configure(wgrad_ct=0)
        E.assert_bits_equal(got.contiguous(), E.cast(ref, torch.float32), 'wgrad {}->{} k{} s{} {}x{}x{} abs {} ct {} {}'.format(
            cin, cout, k, stride, N, H, W, x_abs, ct, kind), layout='nchw')


# --------------------------------------------------------------------------------------------- #
# window-plane, streaming and weights-in-registers kernels
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('half', ['0', '1'])
@pytest.mark.parametrize('cin,cout,HW,N,stride', [
    (64, 128, 28, 1, 1), (128, 128, 28, 3, 1),      # four 7-row tiles per image
    (64, 256, 14, 1, 1), (128, 128, 14, 3, 1),      # one image per tile
    (64, 128, 7, 1, 1), (64, 128, 7, 4, 1), (128, 384, 7, 5, 1), (64, 128, 7, 3, 1),   # four images per tile: a lone image, one tile, one more, one less
    (32, 128, 56, 1, 2), (64, 256, 56, 3, 2),
    (32, 128, 28, 1, 2), (96, 128, 28, 3, 2),
    (32, 128, 14, 1, 2), (32, 128, 14, 4, 2), (64, 384, 14, 5, 2), (32, 256, 14, 3, 2),
])
def test_conv3x3_win_exact(S, dev, monkeypatch, kind, half, cin, cout, HW, N, stride):
    """Stride 1 and 2, with and without bias, ReLU and the ReLU-gradient mask; whole and half tiles (SC2_WIN_HALF)."""
    hip = S.hip
    monkeypatch.setenv('SC2_WIN_HALF', half)
    assert hip.conv3x3_win_supported(HW, HW, cin, cout, 3, 3, stride, 1)
    g, K, x, w = operands(kind, cin, cout, 3, HW, HW, N, seed=stride)
    bias = E.bias_ints(cout, g)
    E.check_bound(K, x, w, bias)
    conv = E.conv_ref(x, w, stride, 1)
    if kind == 'narrow':
        E.check_narrow(conv)
    mask = E.residual_ints(tuple(conv.shape), g)
    xd, wf = X(x, dev), A(hip.pack_conv3x3_win(w.to(dev)), dev)
    bd, zd = A(bias, dev), A(torch.zeros(cout), dev)
    tag = '3x3 win {}->{} {}x{} N {} s{} half {} {}'.format(cin, cout, HW, HW, N, stride, half, kind)
    for b, bt, relu in ((None, zd, False), (bias, bd, False), (bias, bd, True), (None, zd, True)):
        got = hip.conv3x3_win_fwd(xd, wf, bt, relu=relu, stride=stride)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, want_nhwc(epilogue(conv, b, relu=relu)), tag + ' bias {} relu {}'.format(b is not None, relu))
    if stride == 1:
        got = hip.conv3x3_win_fwd(xd, wf, bd, mask=X(mask, dev))
        torch.cuda.synchronize()
        E.assert_bits_equal(got, want_nhwc(epilogue(conv, bias, mask=mask)), tag + ' relu-gradient mask')


@pytest.mark.parametrize('kind', KINDS)
def test_conv3x3_win_dilated_phase_grid(S, dev, kind):
    """The dilated phase-grid use: a dilation-2 3x3 conv on a 28 x 28 map is four stride-1 convs on its 14 x 14 phases."""
    hip = S.hip
    cin, cout, N = 64, 128, 3
    g, K, x, w = operands(kind, cin, cout, 3, 28, 28, N)
    bias = E.bias_ints(cout, g)
    E.check_bound(K, x, w, bias)
    conv = E.conv_ref(x, w, 1, 2, 2)
    if kind == 'narrow':
        E.check_narrow(conv)
    ref = epilogue(conv, bias, relu=True)
    wf, bd = A(hip.pack_conv3x3_win(w.to(dev)), dev), A(bias, dev)
    got = torch.empty(N, 28, 28, cout, dtype=BF16)
    for a in range(2):
        for b in range(2):
            y = hip.conv3x3_win_fwd(X(x[:, :, a::2, b::2], dev), wf, bd, relu=True)
            torch.cuda.synchronize()
            got[:, a::2, b::2] = y.cpu()
    E.assert_bits_equal(got, want_nhwc(ref), 'dilated 3x3 as four phase grids ' + kind)


def _conv1x1_case(S, dev, kind, fwd, pack, cin, cout, stride, N, H, W, res, relu, mask, tag):
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, 1, H, W, N, seed=stride)
    bias = E.bias_ints(cout, g)
    conv = E.conv_ref(x, w, stride, 0)
    if kind == 'narrow':
        E.check_narrow(conv)
    r = E.residual_ints(tuple(conv.shape), g) if res else None
    m = E.residual_ints(tuple(conv.shape), g) if mask else None
    E.check_bound(K, x, w, bias, r)
    kw = {}
    if res:
        kw['residual'] = X(r, dev)
    if mask:
        kw['mask'] = X(m, dev)
    got = fwd(X(x, dev), A(pack(w.to(dev)), dev), A(bias, dev), stride=stride, relu=relu, **kw)
    torch.cuda.synchronize()
    E.assert_bits_equal(got, want_nhwc(epilogue(conv, bias, r, relu=relu, mask=m)),
                        '{} {}->{} s{} {}x{}x{} res {} relu {} mask {} {}'.format(tag, cin, cout, stride, N, H, W, res, relu, mask, kind))
    return got


WIN1 = [
    # (cin, cout, stride, N, H, W, res, relu, mask)            208-pixel tiles
    (1024, 256, 1, 1, 14, 14, False, True, False), (1024, 256, 1, 3, 14, 14, False, True, False),
    (128, 128, 1, 1, 1, 207, False, False, False), (128, 128, 1, 1, 1, 208, True, True, False), (128, 128, 1, 1, 1, 209, False, True, False),
    (256, 384, 1, 3, 5, 30, True, True, False),      # rows of 30 straddle tiles, image borders at 150 / 300 inside tiles
    (128, 128, 1, 1, 1, 1, True, False, False),      # one pixel
    (512, 2048, 1, 1, 7, 7, True, True, False),      # 16 channel chunks
    (1024, 2048, 2, 3, 14, 14, False, False, False), (256, 128, 2, 1, 5, 5, False, True, False), (128, 256, 2, 3, 28, 29, True, True, False),
    (512, 128, 1, 3, 9, 9, False, False, True), (512, 256, 1, 1, 15, 14, True, False, True), (2048, 512, 1, 1, 7, 7, False, False, True),
]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,stride,N,H,W,res,relu,mask', WIN1)
def test_conv1x1_win_exact(S, dev, monkeypatch, kind, cin, cout, stride, N, H, W, res, relu, mask):
    hip = S.hip
    assert hip.conv1x1_win_supported(cin, cout, 1, 1, stride, 0)
    pack = lambda w: hip.pack_conv_win(w)      # noqa: E731
    ref = _conv1x1_case(S, dev, kind, hip.conv1x1_win_fwd, pack, cin, cout, stride, N, H, W, res, relu, mask, '1x1 win')
    for name, value in (('SC2_P1_HALF', '1'), ('SC2_P1_NBUF', '2'), ('SC2_P1_NBUF', '4')):      # 112-pixel tiles; both ring depths
        monkeypatch.setenv(name, value)
        got = _conv1x1_case(S, dev, kind, hip.conv1x1_win_fwd, pack, cin, cout, stride, N, H, W, res, relu, mask, '1x1 win ' + name + value)
        assert torch.equal(got, ref)
        monkeypatch.delenv(name)


STREAM = [
    # (cin, cout, stride, N, H, W, res, relu, mask)        128-pixel units (K = 512: 64)
    (128, 512, 1, 1, 28, 28, True, True, False), (256, 1024, 1, 3, 14, 14, True, True, False),
    (64, 256, 1, 1, 1, 127, False, True, False), (64, 128, 1, 1, 1, 128, True, False, False), (128, 128, 1, 1, 1, 129, False, True, False),
    (256, 128, 1, 1, 1, 128, False, False, False), (256, 256, 1, 1, 1, 129, True, True, False),
    (512, 256, 1, 1, 1, 63, False, True, False), (512, 128, 1, 1, 1, 64, True, True, False), (512, 384, 1, 1, 1, 65, False, False, False),
    (256, 384, 1, 3, 6, 25, True, True, False),      # K = 256 with 128-channel units and a residual
    (128, 384, 1, 3, 6, 25, True, True, False),      # rows of 25 straddle units, image borders at 150 / 300 inside units; Cout % 256 != 0
    (64, 128, 1, 1, 1, 1, False, False, False),
    (256, 512, 2, 3, 13, 10, False, False, False), (512, 256, 2, 1, 15, 15, True, True, False), (128, 128, 2, 1, 1, 1, False, True, False),
    (128, 512, 1, 3, 9, 11, True, False, True), (256, 1024, 1, 1, 14, 14, False, False, True), (128, 256, 1, 1, 1, 129, True, False, True),
]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,stride,N,H,W,res,relu,mask', STREAM)
def test_conv1x1_stream_exact(S, dev, kind, cin, cout, stride, N, H, W, res, relu, mask):
    hip = S.hip
    assert hip.conv1x1_stream_supported(cin, cout, 1, 1, stride, 0)
    assert not mask or hip.conv1x1_stream_mask_supported(cin, cout, stride)
    pack = lambda w: hip.pack_weight_fragments(w.reshape(cout, cin))      # noqa: E731
    _conv1x1_case(S, dev, kind, hip.conv1x1_stream_fwd, pack, cin, cout, stride, N, H, W, res, relu, mask, '1x1 stream')


KRES = [
    # (cin, cout, stride, N, H, W, relu)          32-pixel units (K = 2048: 16)
    (1024, 256, 1, 1, 14, 14, True), (1024, 512, 1, 3, 14, 14, False),
    (1024, 128, 1, 1, 1, 31, True), (1024, 128, 1, 1, 1, 32, False), (1024, 128, 1, 1, 1, 33, True),
    (2048, 64, 1, 1, 1, 15, True), (2048, 64, 1, 1, 1, 16, False), (2048, 128, 1, 1, 1, 17, True),
    (1024, 384, 1, 3, 3, 13, True),       # rows of 13 straddle units, image borders at 39 / 78 inside units
    (1024, 2048, 2, 3, 14, 14, False), (2048, 512, 1, 1, 7, 7, True), (2048, 192, 2, 3, 5, 6, True), (1024, 128, 2, 1, 1, 1, False),
]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,stride,N,H,W,relu', KRES)
def test_conv1x1_kres_exact(S, dev, kind, cin, cout, stride, N, H, W, relu):
    hip = S.hip
    assert bool(hip.lib().sc2_conv1x1_kres_supported(cin, cout, stride))
    pack = lambda w: hip.pack_weight_fragments(w.reshape(cout, cin))      # noqa: E731
    fwd = lambda x, w, b, stride, relu: hip.conv1x1_kres_fwd(x, w, b, stride=stride, relu=relu)      # noqa: E731
    _conv1x1_case(S, dev, kind, fwd, pack, cin, cout, stride, N, H, W, False, relu, False, '1x1 kres')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N,H,W,N2', [(1, 28, 28, 128), (3, 28, 28, 256), (1, 1, 111, 128), (1, 1, 112, 256), (1, 1, 113, 128), (3, 5, 30, 256),
                                      (1, 1, 1, 128)])
def test_conv1x1_pair_exact(S, dev, kind, N, H, W, N2):
    """conv3 (+ residual + ReLU) and the next block's conv1 (+ ReLU) in one launch against the two-step integer reference with the
    intermediate cast to bf16; 112-pixel tiles."""
    hip = S.hip
    K1, C = 128, 512
    assert hip.conv1x1_pair_supported(K1, C, N2)
    g, _, o, w3 = operands(kind, K1, C, 1, H, W, N, seed=N2)
    w1 = E.operand(kind, (N2, C, 1, 1), C, g)
    b3, b1 = E.bias_ints(C, g), E.bias_ints(N2, g)
    ident = E.residual_ints((N, C, H, W), g)
    E.check_bound(K1, o, w3, b3, ident)
    c3 = E.conv_ref(o, w3)
    if kind == 'narrow':
        E.check_narrow(c3)      # (the second stage's operand h is then a bf16-exact integer; its own outputs run higher: f32-exact)
    h64 = epilogue(c3, b3, ident, relu=True)
    h = E.cast(h64, BF16)                                       # the intermediate is stored (and read back) as bf16
    assert float(h.float().abs().max()) * C * float(w1.abs().max()) + 4 < E.EXACT_LIMIT
    u64 = epilogue(E.conv_ref(h.float(), w1), b1, relu=True)
    hd, ud = hip.conv1x1_pair_fwd(X(o, dev), A(hip.pack_weight_fragments(w3.reshape(C, K1).to(dev)), dev), A(b3, dev), X(ident, dev),
                                  A(hip.pack_weight_fragments(w1.reshape(N2, C).to(dev)), dev), A(b1, dev))
    torch.cuda.synchronize()
    E.assert_bits_equal(hd, E.nhwc(h), 'pair h {}x{}x{} N2 {} {}'.format(N, H, W, N2, kind))
    E.assert_bits_equal(ud, want_nhwc(u64), 'pair u {}x{}x{} N2 {} {}'.format(N, H, W, N2, kind))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,pad,N,H,W,run', [
    (512, 0, 1, 56, 56, 0), (256, 1, 1, 55, 55, 0),      # the static geometries at the operating point
    (64, 0, 3, 9, 56, 3), (128, 1, 3, 6, 55, 5),         # odd N, joined runs of tiles
    (64, 0, 1, 5, 56, 0), (64, 0, 1, 6, 56, 0), (64, 0, 1, 4, 56, 0),      # 4 output rows = one tile, one more, one less
    (64, 0, 3, 5, 2, 0), (64, 1, 3, 1, 1, 0),            # the narrowest maps
    (128, 0, 1, 6, 111, 0), (64, 1, 1, 7, 56, 0), (64, 0, 1, 3, 57, 0), (64, 1, 1, 3, 129, 0),      # any width: segments of 55 columns
])
def test_conv2x2_win_exact(S, dev, monkeypatch, kind, cin, pad, N, H, W, run):
    """pad 0 and pad 1, any width, and (pad 1) out= with both channel0 halves of a 512-channel tensor."""
    hip = S.hip
    if run:
        monkeypatch.setenv('SC2_W2_RUN', str(run))
    g, K, x, w = operands(kind, cin, 256, 2, H, W, N, seed=pad)
    E.check_bound(K, x, w)
    assert hip.conv2x2_win_supported((N, H, W, cin), 256, 2, 2, 1, pad)
    ref = E.conv_ref(x, w, 1, pad)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd, wf = X(x, dev), A(hip.pack_conv2x2_win(w.to(dev)), dev)
    tag = '2x2 win {} p{} {}x{}x{} run {} {}'.format(cin, pad, N, H, W, run, kind)
    OH, OW = ref.shape[2:]
    got = hip.conv2x2_win_fwd(xd, wf, pad)
    torch.cuda.synchronize()
    E.assert_bits_equal(got, want_nhwc(ref), tag)
    if pad == 1:
        w2 = E.operand(kind, (256, cin, 2, 2), K, g)
        ref2 = E.conv_ref(x, w2, 1, 1)
        out = E.arena_like((N, OH, OW, 512), BF16, dev)
        hip.conv2x2_win_fwd(xd, wf, 1, out=out, channel0=0)
        torch.cuda.synchronize()
        E.assert_bits_equal(out[..., :256], want_nhwc(ref), tag + ' channel0 0')
        assert bool(torch.isnan(out[..., 256:].float()).all()), 'the other half was written'
        hip.conv2x2_win_fwd(xd, A(hip.pack_conv2x2_win(w2.to(dev)), dev), 1, out=out, channel0=256)
        torch.cuda.synchronize()
        E.assert_bits_equal(out, want_nhwc(torch.cat([ref, ref2], 1)), tag + ' both halves')
        E.assert_bands_untouched(out, tag + ' out=')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N,run,want_y', [(1, 0, True), (3, 5, False)])
def test_conv2x2_win_tail_exact(S, dev, monkeypatch, kind, N, run, want_y):
    """The last decoder conv with layer2.0's conv1 (+ ReLU) and downsample (stride 2) behind it: three-step integer reference, the
    conv output cast to bf16 in between."""
    hip = S.hip
    if run:
        monkeypatch.setenv('SC2_W2_RUN', str(run))
    g, K, x, w4 = operands(kind, 256, 256, 2, 55, 55, N)
    w1 = E.operand(kind, (128, 256, 1, 1), 256, g)
    wds = E.operand(kind, (512, 256, 1, 1), 256, g)
    b1, bds = E.bias_ints(128, g), E.bias_ints(512, g)
    E.check_bound(K, x, w4)
    assert hip.conv2x2_win_tail_supported((N, 55, 55, 256))
    y64 = E.conv_ref(x, w4, 1, 1)
    if kind == 'narrow':
        E.check_narrow(y64)
    y = E.cast(y64, BF16)
    assert float(y.float().abs().max()) * 256 * 3 + 4 < E.EXACT_LIMIT
    o1 = epilogue(E.conv_ref(y.float(), w1), b1, relu=True)
    ods = epilogue(E.conv_ref(y.float(), wds, 2, 0), bds)
    stream = A(hip.pack_conv2x2_win_tail(w4.to(dev), w1.reshape(128, 256).to(dev).to(BF16), wds.reshape(512, 256).to(dev).to(BF16)), dev)
    g1, gds, gy = hip.conv2x2_win_tail_fwd(X(x, dev), stream, A(b1, dev), A(bds, dev), want_y=want_y)
    torch.cuda.synchronize()
    tag = '2x2 win tail N {} run {} {}'.format(N, run, kind)
    E.assert_bits_equal(g1, want_nhwc(o1), tag + ' conv1')
    E.assert_bits_equal(gds, want_nhwc(ods), tag + ' downsample')
    if want_y:
        E.assert_bits_equal(gy, E.nhwc(y), tag + ' y')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cout,N,H,W', [(24, 1, 56, 56), (24, 3, 9, 7), (32, 1, 2, 17), (16, 1, 2, 18), (8, 1, 2, 16), (1, 5, 2, 2), (24, 3, 5, 9)])
def test_conv2x2_c48_exact(S, dev, kind, cout, N, H, W):
    """f32 latent and, with medians that are multiples of 0.25, the symbols; 16-pixel tiles (1 x 16: one tile, 15, 17); out=."""
    hip = S.hip
    g, K, x, w = operands(kind, 48, cout, 2, H, W, N)
    med = E.quarter_medians(cout, g)
    E.check_bound(K, x, w)
    assert hip.conv2x2_c48_supported((N, H, W, 48), cout, 2, 2, 1, 0)
    ref = E.conv_ref(x, w)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd, wf = X(x, dev), A(hip.pack_conv2x2_c48(w.to(dev)), dev)
    tag = '2x2 c48 cout {} {}x{}x{} {}'.format(cout, N, H, W, kind)
    out = E.arena_like(tuple(ref.shape), torch.float32, dev)
    lat = hip.conv2x2_c48_fwd(xd, wf, cout, out=out)
    torch.cuda.synchronize()
    E.assert_bits_equal(lat, E.cast(ref, torch.float32), tag + ' latent', layout='nchw')
    E.assert_bands_untouched(out, tag + ' latent')
    out = E.arena_like(tuple(ref.shape), torch.int32, dev)
    sym = hip.conv2x2_c48_fwd(xd, wf, cout, medians=A(med, dev), out=out)
    torch.cuda.synchronize()
    E.assert_bits_equal(sym, E.cast(torch.round(ref - med.double().view(1, -1, 1, 1)), torch.int32), tag + ' symbols', layout='nchw')
    E.assert_bands_untouched(out, tag + ' symbols')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('M,K,N', [(127, 2048, 1008), (128, 512, 32), (129, 128, 16), (1, 128, 32), (5, 256, 48), (3, 4608, 16)])
def test_fc_exact(S, dev, kind, M, K, N):
    """The classifier GEMM (K a multiple of 128): 128-row tiles; K = 128 is its shortest loop."""
    hip = S.hip
    g = E.gen(M, K, N, kind == 'wide')
    a, w = E.operand(kind, (M, K), K, g), E.operand(kind, (N, K), K, g)
    bias = E.bias_ints(N, g)
    E.check_bound(K, a, w, bias)
    prod = a.double() @ w.double().t()
    if kind == 'narrow':
        E.check_narrow(prod)
    ref = prod + bias.double()
    got = hip.fc_fwd(A(a.to(BF16), dev), A(hip.pack_weight_fragments(w.to(dev)), dev), A(bias, dev))
    torch.cuda.synchronize()
    E.assert_bits_equal(got, E.cast(ref, torch.float32), 'fc {}x{}x{} {}'.format(M, K, N, kind))


# --------------------------------------------------------------------------------------------- #
# f32 and split-bf16 encoder convolutions: an integer's bf16 split has zero second and third parts
# --------------------------------------------------------------------------------------------- #
PRECISE = [
    # (cin, cout, k, s, p, H, W, N)                   128-pixel tiles, chunks of 32 / 48 / 96 channels
    (4, 96, 5, 2, 2, 37, 50, 1), (96, 48, 5, 2, 2, 28, 31, 3), (48, 24, 2, 1, 0, 13, 9, 3),
    (8, 200, 3, 1, 1, 10, 12, 1),       # three chunks, the last partial
    (4, 5, 1, 1, 0, 1, 127, 1), (4, 32, 1, 1, 0, 1, 128, 1), (4, 48, 1, 1, 0, 1, 129, 1),
    (8, 40, 3, 1, 1, 7, 50, 3),         # rows straddle tiles, image borders inside tiles
    (12, 96, 3, 1, 1, 1, 1, 1),         # 1 x 1 map, k > H
    (20, 20, 1, 2, 0, 5, 5, 1),         # K = 20: one k-step of 32 / two of 16 with a tail
]


def _precise(S, mode):
    hip = S.hip
    if mode == 'f32':
        return hip.pack_conv_f32, hip.conv2d_f32_fwd
    ns = 2 if mode == 'bf16x3' else 3
    return (lambda w: hip.pack_conv_split(w, ns)), (lambda *a, **k: hip.conv2d_split_fwd(*a, ns=ns, **k))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cin,cout,k,s,p,H,W,N', PRECISE)
def test_precise_convs_equal_the_integer_conv(S, dev, kind, cin, cout, k, s, p, H, W, N):
    """'f32', 'bf16x3' and 'bf16x6' all equal the integer result, hence each other: three output formats, bias, symbols."""
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, k, H, W, N)
    bias, med = E.bias_ints(cout, g), E.quarter_medians(cout, g)
    E.check_bound(K, x, w, bias)
    ref = E.conv_ref(x, w, s, p)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd = X(x, dev, torch.float32)
    bd, md = A(bias, dev), A(med, dev)
    for mode in ('f32', 'bf16x3', 'bf16x6'):
        pack, fwd = _precise(S, mode)
        wf = A(pack(w.to(dev)), dev)
        tag = '{} {}->{} k{} s{} {}x{}x{} {}'.format(mode, cin, cout, k, s, N, H, W, kind)
        got = fwd(xd, wf, cout, k, k, s, p)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, want_nhwc(ref, torch.float32), tag + ' nhwc')
        got = fwd(xd, wf, cout, k, k, s, p, out_format=hip.OUT_F32_NCHW)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, E.cast(ref, torch.float32), tag + ' nchw', layout='nchw')
        got = fwd(xd, wf, cout, k, k, s, p, out_format=hip.OUT_F32_NCHW, epilogue=hip.EPI_BIAS, ep_beta=bd)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, E.cast(epilogue(ref, bias), torch.float32), tag + ' + bias', layout='nchw')
        out = E.arena_like(tuple(ref.shape), torch.int32, dev)
        got = fwd(xd, wf, cout, k, k, s, p, out_format=hip.OUT_I32_NCHW_SYM, ep_beta=md, out=out)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, E.cast(torch.round(ref - med.double().view(1, -1, 1, 1)), torch.int32), tag + ' symbols', layout='nchw')
        E.assert_bands_untouched(out, tag + ' symbols')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('a_op', ['abs', 'square'])
@pytest.mark.parametrize('cin,cout,k,H,W,N', [(96, 96, 1, 9, 11, 3), (48, 48, 1, 1, 129, 1), (20, 20, 1, 7, 5, 1), (8, 200, 3, 10, 12, 1)])
def test_precise_convs_operand_ops(S, dev, kind, a_op, cin, cout, k, H, W, N):
    """AOP_ABS / AOP_SQUARE (the operand forms of the GDN1 / GDN gamma GEMMs) without an epilogue: |x| and x^2 of small integers are
    integers, so all three modes equal conv(|x|, w) / conv(x^2, w)."""
    hip = S.hip
    g, K, x, w = operands(kind, cin, cout, k, H, W, N, seed=len(a_op))
    xa = x.abs() if a_op == 'abs' else x * x
    E.check_bound(K, xa, w)
    ref = E.conv_ref(xa, w, 1, k // 2)
    if kind == 'narrow':
        E.check_narrow(ref)
    xd = X(x, dev, torch.float32)
    for mode in ('f32', 'bf16x3', 'bf16x6'):
        pack, fwd = _precise(S, mode)
        got = fwd(xd, A(pack(w.to(dev)), dev), cout, k, k, 1, k // 2, a_op=hip.AOP_ABS if a_op == 'abs' else hip.AOP_SQUARE)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, want_nhwc(ref, torch.float32), '{} a_op {} {}->{} k{} {}'.format(mode, a_op, cin, cout, k, kind))


# --------------------------------------------------------------------------------------------- #
# GDN1 with a live gamma, bit for bit: the arithmetic each kernel family documents
# --------------------------------------------------------------------------------------------- #
F32 = torch.float32
# family -> (precision in which t = the conv output enters the second GEMM as |t|, precision in which it enters the final product,
#            the reciprocal of the forward form).  'ieee': r = 1.0f / n, correctly rounded, then ONE multiply t * r -- restated on the
# CPU by exact_ints.gdn_restate and compared with assert_bits_equal; 'rcpf': the hardware reciprocal (within 1 ulp), compared with
# assert_bits_in against exact_ints.gdn_admissible.  The inverse form is t * n in every family (one f32 multiply).  Each row is what
# the family's own comment states, csrc/ file and line of that comment:
GDN_FAMILIES = {
    # conv_fused_gdn_small: "|x| enters the second GEMM rounded to bf16, the product takes the unrounded f32 x", "IEEE division, then one multiply"
    'small tiles': (BF16, F32, 'ieee'),           # conv_igemm_impl.h:534-539; code: pack_bf16x2(acc) & 0x7FFF7FFF -> Xi; acc * (1.0f / norm)
    # conv_store_tile / conv_store_tile_f32 with SC2_EPI_GDN / _IGDN: ep_x is the caller's bf16 tensor, read for the GEMM (a_op ABS) and the product
    'tile epilogue': (BF16, BF16, 'ieee'),        # conv_igemm_impl.h:537-538; code: xv[t] * (1.0f / norm) at 269, 476, 511
    # the 256-wide tiles and their persistent form: "x is the image's bf16 value in both places", "IEEE division, then one multiply"
    '256-wide tiles': (BF16, BF16, 'ieee'),       # conv_igemm_impl.h:1002-1005 ("x goes to an LDS image as bf16 ... x read back from the image"), conv_dec_persist.hip:401-403
    # "t is rounded to bf16 into the LDS IMAGE", "t is the image's bf16 value here as in phase 2", "IEEE division then one multiply"
    'conv_gdn512': (BF16, BF16, 'ieee'),          # conv_gdn512.hip:13-21
    # "x read back from the lane's own image slots -- the bf16 value in both places", "IEEE division then one multiply"
    'conv2x2_win': (BF16, BF16, 'ieee'),          # conv2x2_win.hip:16-20
    # modes f32, bf16x3, bf16x6: "norm = gamma |x| consumes [the accumulators] in place" (f32) / "norm = gamma |acc| as a split GEMM"; the
    # one epilogue: "norm = beta + acc, IEEE division, one multiply"
    'precise': (F32, F32, 'ieee'),                # conv_precise.h:6-8, conv_f32.hip:263-267, conv_split.hip:211-212
    # "|t| enters it ROUNDED TO bf16", "y = t * rcp(norm) with t the f32 accumulator and rcp the hardware reciprocal"
    'conv0_gdn96': (BF16, F32, 'rcpf'),           # conv0_gdn96.hip:14-18
    'conv2_gdn48': (BF16, F32, 'rcpf'),           # conv2_gdn48.hip:20-23
}

FUSED_PRECISE = [(4, 96, 5, 2, 2, 21, 18, 3), (96, 48, 5, 2, 2, 9, 30, 1), (8, 32, 3, 1, 1, 1, 129, 1), (4, 20, 1, 1, 0, 7, 5, 1)]
FIRST_STAGE = [(1, 224, 224), (3, 9, 14), (1, 2, 62), (1, 2, 64), (1, 2, 66), (1, 1, 2)]
FUSED_SMALL = [(96, 48, 5, 2, 2, 13, 10, 3), (16, 96, 3, 1, 1, 1, 129, 1), (24, 64, 2, 1, 1, 7, 9, 1), (8, 32, 1, 1, 0, 1, 1, 1)]
FUSED_BIG = [(512, 2, 0, 11, 10, 3), (64, 1, 0, 1, 257, 1), (256, 2, 1, 15, 15, 1)]
CONV0_GDN96 = [(1, 224, 224), (3, 11, 224), (1, 5, 226), (1, 4, 2), (3, 6, 40), (1, 3, 448)]
CONV2_GDN48 = [(1, 112, 112), (3, 9, 112), (1, 3, 111), (1, 4, 113), (1, 1, 1), (3, 5, 30), (1, 2, 257)]
GDN512 = [(24, 1, 27, 27), (24, 3, 7, 9), (16, 1, 1, 126), (8, 1, 1, 127), (24, 1, 1, 128), (8, 1, 1, 1), (16, 3, 5, 20)]
WIN_FUSED = [(512, 0, 1, 56, 56), (128, 1, 3, 6, 55), (64, 0, 1, 5, 111), (64, 1, 3, 1, 1), (64, 0, 1, 6, 57)]
TILE_EPILOGUE = [(C, M) for C in (48, 40) for M in (1, 128, 129)]
# test -> (family, cases, case -> (cin, cout, k, stride, pad, H, W, N) of the convolution in front of the GDN1).  tests/test_exact_ints_cpu.py
# walks this table: what it proves on the CPU, it proves for the operands the tests below hand to the kernels.
GDN_TESTS = {
    'test_precise_fused_gdn_exact': ('precise', FUSED_PRECISE, lambda c: c),
    'test_precise_first_stage_on_the_image': ('precise', FIRST_STAGE, lambda c: (3, 96, 5, 2, 2, c[1], c[2], c[0])),
    'test_conv2d_fused_gdn_small_tiles_exact': ('small tiles', FUSED_SMALL, lambda c: c),
    'test_conv2d_fused_gdn_big_tile_exact': ('256-wide tiles', FUSED_BIG, lambda c: (c[0], 256, c[1], 1, c[2], c[3], c[4], c[5])),
    'test_conv0_gdn96_exact': ('conv0_gdn96', CONV0_GDN96, lambda c: (3, 96, 5, 2, 2, c[1], c[2], c[0])),
    'test_conv2_gdn48_exact': ('conv2_gdn48', CONV2_GDN48, lambda c: (96, 48, 5, 2, 2, c[1], c[2], c[0])),
    'test_conv2x2_gdn512_exact': ('conv_gdn512', GDN512, lambda c: (c[0], 512, 2, 1, 1, c[2], c[3], c[1])),
    'test_conv2x2_win_fused_gdn_exact': ('conv2x2_win', WIN_FUSED, lambda c: (c[0], 256, 2, 1, c[1], c[3], c[4], c[2])),
    'test_gdn1_tile_epilogue_exact': ('tile epilogue', TILE_EPILOGUE, None),
}


# (test, case, kind, inverse) -> another seed, where test_exact_ints_cpu.py found the first one's operands blind to one of its mutants:
# at the single output pixel of a 1 x 1 / 1 x 2 map, swapping gamma's first two columns did not change the expected bits
GDN_RESEED = {('test_precise_first_stage_on_the_image', (1, 1, 2), 'narrow', True): 1}


def gdn_case(test, kind, inverse, case):
    """-> (family, x, w, t, params): the operands of one case of one test above, its exact conv output t (f64 NCHW) and the
    (gamma, beta, label) variants -- drawn ONCE per case, after the operands, from the case's generator.  (The stand-alone GDN1 has no
    conv: x is then the integer tensor before its rounding to bf16, the operand of the precise modes' launches, and w is None.)"""
    family, _, geom = GDN_TESTS[test]
    if geom is None:                 # the stand-alone GDN1: t IS the bf16 input tensor [1, C, 1, M]
        C, M = case
        g = E.gen(C, M, inverse, kind == 'wide')
        t = torch.randint(-4000, 4001, (1, C, 1, M), generator=g) if kind == 'wide' else torch.randint(-256, 257, (1, C, 1, M), generator=g)
        x = t.double()                           # the integers themselves (wide: not bf16-exact): what the precise modes take as f32
        t = t.float().to(BF16).double()          # wide: integers rounded to bf16 (still integers); narrow: |t| <= 256 is bf16-exact
        w = None
        cout = C
    else:
        cin, cout, k, s, p, H, W, N = geom(case)
        kh, kw = (k, k) if isinstance(k, int) else k
        g, K, x, w = operands(kind, cin, cout, k, H, W, N, seed=int(inverse) + 2 * GDN_RESEED.get((test, case, kind, inverse), 0))
        live = cin * min(kh, H) * min(kw, W)                    # the taps that can lie inside the map: a 1 x 1 map under a 5 x 5 filter has one
        if kind == 'wide' and E.wide_amplitude(live) != 3:      # short K: larger integers, so that |t| leaves the bf16-exact integers
            x, w = E.wide_to(x.shape, E.wide_amplitude(live), g), E.wide_to(w.shape, E.wide_amplitude(live), g)
        if kind == 'narrow' and E.narrow_amplitude(live) != 1:   # short K: a few more values, so that |t| is not a handful of powers of two
            x, w = E.wide_to(x.shape, E.narrow_amplitude(live), g), E.wide_to(w.shape, E.narrow_amplitude(live), g)
        E.check_bound(K, x, w)
        t = E.conv_ref(x, w, s, p)
    if kind == 'narrow':
        E.check_narrow(t)
    params = E.gdn_params(kind, cout, g, inverse, tmax=float(t.abs().max()))
    return family, x, w, t, params


def gdn_restated(family, t, gamma, beta, inverse, dtype):
    t_gemm, t_prod, _ = GDN_FAMILIES[family]
    return E.gdn_restate(t, gamma, beta, inverse, t_gemm, t_prod, dtype)


def assert_gdn(family, got_nhwc, t, gamma, beta, inverse, label, what):
    """bf16 / f32 NHWC output of one launch against the family's restatement: bit-equal, but for the forward live-gamma form of the two
    hardware-reciprocal kernels, which must hit one of the admissible values (a single one almost everywhere: test_exact_ints_cpu.py)."""
    t_gemm, t_prod, rcp = GDN_FAMILIES[family]
    if rcp == 'rcpf' and not inverse and label == 'live gamma':
        cands, _ = E.gdn_admissible(t, gamma, beta, t_gemm, t_prod, got_nhwc.dtype)
        E.assert_bits_in(got_nhwc, [E.nhwc(c) for c in cands], what)
    else:
        E.assert_bits_equal(got_nhwc, E.nhwc(E.gdn_restate(t, gamma, beta, inverse, t_gemm, t_prod, got_nhwc.dtype)), what)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('cin,cout,k,s,p,H,W,N', FUSED_PRECISE)
def test_precise_fused_gdn_exact(S, dev, kind, inverse, cin, cout, k, s, p, H, W, N):
    hip = S.hip
    family, x, w, t, params = gdn_case('test_precise_fused_gdn_exact', kind, inverse, (cin, cout, k, s, p, H, W, N))
    xd = X(x, dev, torch.float32)
    for mode in ('f32', 'bf16x3', 'bf16x6'):
        pack, fwd = _precise(S, mode)
        wf = A(pack(w.to(dev)), dev)
        for gamma, beta, label in params:
            got = fwd(xd, wf, cout, k, k, s, p, epilogue=hip.EPI_FUSED_IGDN if inverse else hip.EPI_FUSED_GDN,
                      ep_x=A(pack(gamma.reshape(cout, cout, 1, 1).to(dev)), dev), ep_beta=A(beta, dev))
            torch.cuda.synchronize()
            assert_gdn(family, got, t, gamma, beta, inverse, label,
                       '{} fused {} {}->{} {} {}'.format(mode, 'IGDN' if inverse else 'GDN', cin, cout, label, kind))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('persist', ['1', '0'])
@pytest.mark.parametrize('N,H,W', FIRST_STAGE)
def test_precise_first_stage_on_the_image(S, dev, monkeypatch, kind, inverse, persist, N, H, W):
    """x_is_nchw_rgb: the f32 NCHW image read in place; conv0 + GDN1(96) as the persistent first stage (32-pixel units: 1 x 31 / 32 /
    33 output pixels) and as its tile form (SC2_F32_PERSIST0=0); the split modes on the same image."""
    hip = S.hip
    monkeypatch.setenv('SC2_F32_PERSIST0', persist)
    family, x, w, t, params = gdn_case('test_precise_first_stage_on_the_image', kind, inverse, (N, H, W))
    xd = A(x, dev)
    wants = [E.nhwc(gdn_restated(family, t, gamma, beta, inverse, F32)) for gamma, beta, _ in params]      # once, shared by the modes
    for mode in ('f32', 'bf16x3', 'bf16x6'):
        pack, fwd = _precise(S, mode)
        wf = A(pack(w.to(dev)), dev)
        got = fwd(xd, wf, 96, 5, 5, 2, 2, x_is_nchw_rgb=True)
        torch.cuda.synchronize()
        E.assert_bits_equal(got, want_nhwc(t, torch.float32), '{} conv0 on the image {}x{}x{} {}'.format(mode, N, H, W, kind))
        for (gamma, beta, label), want in zip(params, wants):
            got = fwd(xd, wf, 96, 5, 5, 2, 2, x_is_nchw_rgb=True, epilogue=hip.EPI_FUSED_IGDN if inverse else hip.EPI_FUSED_GDN,
                      ep_x=A(pack(gamma.reshape(96, 96, 1, 1).to(dev)), dev), ep_beta=A(beta, dev))
            torch.cuda.synchronize()
            E.assert_bits_equal(got, want, '{} first stage persist {} {}x{}x{} {} {}'.format(mode, persist, N, H, W, label, kind))


# --------------------------------------------------------------------------------------------- #
# fused conv + GDN1 launches of the bf16 families
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('cin,cout,k,s,p,H,W,N', FUSED_SMALL)
def test_conv2d_fused_gdn_small_tiles_exact(S, dev, kind, inverse, cin, cout, k, s, p, H, W, N):
    """EPI_FUSED_GDN / _IGDN of the 32 / 48 / 64 / 96-row tiles, f32 and bf16 outputs."""
    hip = S.hip
    family, x, w, t, params = gdn_case('test_conv2d_fused_gdn_small_tiles_exact', kind, inverse, (cin, cout, k, s, p, H, W, N))
    xd, wp = X(x, dev), A(hip.pack_conv_weight(w.to(dev)), dev)
    assert hip.conv_fused_gdn_supported(tuple(xd.shape), cout, k, k, s, p) == 1
    for gamma, beta, label in params:
        gd = A(hip.pack_conv_weight(gamma.reshape(cout, cout, 1, 1).to(dev)), dev)
        for fmt in (hip.OUT_BF16_NHWC, hip.OUT_F32_NCHW):
            conv2d(S, dev, xd, wp, cout, k, s, p, t,
                   'fused {} {}->{} fmt {} {} {}'.format('IGDN' if inverse else 'GDN', cin, cout, fmt, label, kind), fmt=fmt,
                   restate=lambda dt: gdn_restated(family, t, gamma, beta, inverse, dt),
                   epilogue=hip.EPI_FUSED_IGDN if inverse else hip.EPI_FUSED_GDN, ep_x=gd, ep_beta=A(beta, dev))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('half', ['0', '1', 'r4'])
@pytest.mark.parametrize('cin,k,pad,H,W,N', FUSED_BIG)
def test_conv2d_fused_gdn_big_tile_exact(S, dev, monkeypatch, kind, inverse, half, cin, k, pad, H, W, N):
    """conv + GDN1(256) in one launch of the 256-wide tiles (forced), the 128-row twins and the 4-wave register tile.  Documented: the
    conv output enters the second GEMM and the final product as bf16 (the LDS image)."""
    hip = S.hip
    monkeypatch.setenv('SC2_CONV_FORCE_BIG', '1')
    monkeypatch.setenv('SC2_CONV_HALF', '0' if half == 'r4' else half)
    monkeypatch.setenv('SC2_CONV_BIG4', '1' if half == 'r4' else '0')
    cout = 256
    family, x, w, t, params = gdn_case('test_conv2d_fused_gdn_big_tile_exact', kind, inverse, (cin, k, pad, H, W, N))
    xd, wp = X(x, dev), A(hip.pack_conv_weight(w.to(dev)), dev)
    assert hip.conv_fused_gdn_supported(tuple(xd.shape), cout, k, k, 1, pad) == 2
    for gamma, beta, label in params:
        gd = A(hip.pack_gamma_fragments(gamma.to(dev)), dev)
        for fmt in (hip.OUT_BF16_NHWC, hip.OUT_F32_NHWC):
            conv2d(S, dev, xd, wp, cout, k, 1, pad, t,
                   'big fused {} {} k{} half {} fmt {} {} {}'.format('IGDN' if inverse else 'GDN', cin, k, half, fmt, label, kind), fmt=fmt,
                   restate=lambda dt: gdn_restated(family, t, gamma, beta, inverse, dt),
                   epilogue=hip.EPI_FUSED_IGDN if inverse else hip.EPI_FUSED_GDN, ep_x=gd, ep_beta=A(beta, dev))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('N,H,W', CONV0_GDN96)
def test_conv0_gdn96_exact(S, dev, kind, inverse, N, H, W):
    """The persistent first stage of the bf16 encoder: 112-pixel output segments (224: the static geometry; 226 -> 112 + 1; a single
    pixel pair; 448 -> two whole segments); y and the emitted conv output t; the in-place NCHW form."""
    hip = S.hip
    family, x, w, t, params = gdn_case('test_conv0_gdn96_exact', kind, inverse, (N, H, W))
    x4 = torch.zeros(N, H, W, 4)
    x4[..., :3] = E.nhwc(x)
    xp = A(x4.to(BF16).view(N, H, W // 2, 8), dev)
    assert hip.conv0_gdn96_supported(tuple(xp.shape), 96)
    wf = A(hip.pack_weight_fragments(hip.pack_conv0_weight_pairs(w.to(dev))[:96]), dev)
    xn = A(x, dev)
    for gamma, beta, label in params:
        gf, bd = A(hip.pack_gamma_fragments(gamma.to(dev)), dev), A(beta, dev)
        tag = 'conv0+gdn96 {}x{}x{} inverse {} {} {}'.format(N, H, W, inverse, label, kind)
        y, tt = hip.conv0_gdn96_fwd(xp, wf, gf, bd, inverse, want_t=True)
        torch.cuda.synchronize()
        assert_gdn(family, y, t, gamma, beta, inverse, label, tag)
        E.assert_bits_equal(tt, want_nhwc(t), tag + ' t')
        y = hip.conv0_gdn96_fwd(xp, wf, gf, bd, inverse)
        torch.cuda.synchronize()
        assert_gdn(family, y, t, gamma, beta, inverse, label, tag + ' (no t)')
        y = hip.conv0_gdn96_nchw_fwd(xn, wf, gf, bd, inverse)
        torch.cuda.synchronize()
        assert_gdn(family, y, t, gamma, beta, inverse, label, tag + ' nchw in place')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('N,H,W', CONV2_GDN48)
def test_conv2_gdn48_exact(S, dev, kind, inverse, N, H, W):
    """The persistent second stage: W = 112 is static, any other width runs 56-column output segments (111 -> 56; 113 -> 56 + 1;
    257 -> 56 + 56 + 17)."""
    hip = S.hip
    family, x, w, t, params = gdn_case('test_conv2_gdn48_exact', kind, inverse, (N, H, W))
    xd = X(x, dev)
    assert hip.conv2_gdn48_supported(tuple(xd.shape), 48, 5, 5, 2, 2)
    wp = A(hip.pack_conv_weight(w.to(dev), hip.K_SLAB_MAJOR | hip.K_B_FRAG_MAJOR), dev)
    for gamma, beta, label in params:
        gf = A(hip.pack_weight_fragments(hip.pack_conv_weight(gamma.reshape(48, 48, 1, 1).to(dev))), dev)
        bd = A(beta, dev)
        tag = 'conv2+gdn48 {}x{}x{} inverse {} {} {}'.format(N, H, W, inverse, label, kind)
        y, tt = hip.conv2_gdn48_fwd(xd, wp, gf, bd, inverse, want_t=True)
        torch.cuda.synchronize()
        assert_gdn(family, y, t, gamma, beta, inverse, label, tag)
        E.assert_bits_equal(tt, want_nhwc(t), tag + ' t')
        y = hip.conv2_gdn48_fwd(xd, wp, gf, bd, inverse)
        torch.cuda.synchronize()
        assert_gdn(family, y, t, gamma, beta, inverse, label, tag + ' (no t)')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('cin,N,H,W', GDN512)
def test_conv2x2_gdn512_exact(S, dev, kind, inverse, cin, N, H, W):
    """decoder[0] + GDN1(512): 128-pixel tiles (2 x 127 = 254, 2 x 128 = 256, 2 x 129 = 258 output pixels)."""
    hip = S.hip
    assert hip.conv2x2_gdn512_supported(cin, 512, 2, 2, 1, 1)
    family, x, w, t, params = gdn_case('test_conv2x2_gdn512_exact', kind, inverse, (cin, N, H, W))
    xd, wp = X(x, dev), A(hip.pack_conv_weight(w.to(dev)), dev)
    for gamma, beta, label in params:
        gf, bd = A(hip.pack_gamma_fragments(gamma.to(dev)), dev), A(beta, dev)
        tag = 'conv2x2+gdn512 {} {}x{}x{} inverse {} {} {}'.format(cin, N, H, W, inverse, label, kind)
        y, tt = hip.conv2x2_gdn512_fwd(xd, wp, gf, bd, inverse, want_t=True)
        torch.cuda.synchronize()
        assert_gdn(family, y, t, gamma, beta, inverse, label, tag)
        E.assert_bits_equal(tt, want_nhwc(t), tag + ' t')
        y = hip.conv2x2_gdn512_fwd(xd, wp, gf, bd, inverse)
        torch.cuda.synchronize()
        assert_gdn(family, y, t, gamma, beta, inverse, label, tag + ' (no t)')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('cin,pad,N,H,W', WIN_FUSED)
def test_conv2x2_win_fused_gdn_exact(S, dev, kind, inverse, cin, pad, N, H, W):
    """conv2x2_win_fwd with beta: the GDN1 behind the decoder conv in the window-plane kernel."""
    hip = S.hip
    family, x, w, t, params = gdn_case('test_conv2x2_win_fused_gdn_exact', kind, inverse, (cin, pad, N, H, W))
    xd = X(x, dev)
    for gamma, beta, label in params:
        wf = A(hip.pack_conv2x2_win(w.to(dev), gamma.to(dev)), dev)
        got = hip.conv2x2_win_fwd(xd, wf, pad, beta=A(beta, dev), inverse=inverse)
        torch.cuda.synchronize()
        assert_gdn(family, got, t, gamma, beta, inverse, label,
                   '2x2 win fused {} p{} {}x{}x{} inverse {} {} {}'.format(cin, pad, N, H, W, inverse, label, kind))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('C,M', TILE_EPILOGUE)
def test_gdn1_tile_epilogue_exact(S, dev, kind, inverse, C, M):
    """The stand-alone GDN1 at widths the resident-row kernels refuse (C = 48: a whole 48-row tile; C = 40: a partial one; M = one
    pixel, one 128-pixel tile, one more): conv2d_fwd(a_op=AOP_ABS, epilogue=EPI_GDN / EPI_IGDN, ep_x=x) with bf16 and f32 outputs, and
    the same launch of the three precise modes (their stand-alone epilogue: f32 in both places) on the f32 tensor of the integers
    BEFORE their rounding to bf16 -- on the wide set most of them are not bf16-exact, so a norm or a product taken from a bf16 value
    would show."""
    hip = S.hip
    family, t32, _, t, params = gdn_case('test_gdn1_tile_epilogue_exact', kind, inverse, (C, M))
    xd = X(t, dev)
    assert torch.equal(xd.cpu().double(), E.nhwc(t))          # t is bf16-exact: the tensor the kernel reads IS t
    assert not hip.gdn1_rows_supported(xd, C)
    assert kind == 'narrow' or not torch.equal(t32, t)
    x32 = X(t32, dev, torch.float32)
    epi = hip.EPI_IGDN if inverse else hip.EPI_GDN
    for gamma, beta, label in params:
        tag = 'GDN1 tile epilogue C {} M {} inverse {} {} {}'.format(C, M, inverse, label, kind)
        gd, bd = A(hip.pack_conv_weight(gamma.reshape(C, C, 1, 1).to(dev)), dev), A(beta, dev)
        for fmt in (hip.OUT_BF16_NHWC, hip.OUT_F32_NHWC, hip.OUT_F32_NCHW):
            conv2d(S, dev, xd, gd, C, 1, 1, 0, t, '{} fmt {}'.format(tag, fmt), fmt=fmt,
                   restate=lambda dt: gdn_restated(family, t, gamma, beta, inverse, dt), a_op=hip.AOP_ABS, epilogue=epi, ep_x=xd, ep_beta=bd)
        for mode in ('f32', 'bf16x3', 'bf16x6'):
            pack, fwd = _precise(S, mode)
            got = fwd(x32, A(pack(gamma.reshape(C, C, 1, 1).to(dev)), dev), C, 1, 1, 1, 0, a_op=hip.AOP_ABS, epilogue=epi, ep_x=x32, ep_beta=bd)
            torch.cuda.synchronize()
            assert_gdn('precise', got, t32, gamma, beta, inverse, label, '{} mode {}'.format(tag, mode))


