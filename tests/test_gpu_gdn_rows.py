"""-m gpu: the resident-row GDN1 kernels -- csrc/gdn512_rows.hip (C = 512 / 256, 128-pixel tiles, one persistent workgroup per CU) and
csrc/gdn96_strips.hip (C = 96, 32-pixel strips, eight independent waves per workgroup) -- element by element against the float64
reference of tests/ref_gdn_rows.py, PAST one tile per workgroup / one strip per wave.  They carry every GDN1 and inverse GDN1 of a
training step; the rest of the suite runs their first trip only (tests/test_gpu_kernels.py::test_gdn512_rows: 1 152, 198 and 5 pixels,
by norm) and everything their persistent loops carry over -- the reused LDS image, the fragment ring, the d_beta sums in registers, the
masks in LDS, the parking stores of tile t against the stream-out of tile t + 1, the strips' per-wave areas -- under
test_gpu_training's norms.

  operands      dyadic (ref_gdn_rows: 'narrow', 'wide' on the inverse form, 'div' on the division form with every norm a power of
                two): every f32 intermediate is exact in any order, so y, d_norm and dx EQUAL reference.to(bfloat16) and d_beta
                the f32 value -- as values (the sign of a zero is left open), nothing non-finite, no tolerance.  The
                conditions are proven on the reference by tests/test_gdn_rows_ref_cpu.py, which also shows what this comparison
                rejects.  The reference of a case is evaluated in float64 on the device (exact integers and dyadics).
  every launch  runs twice: once through hip.gdn1_rows_fwd / hip.gdn1_rows_bwd, once through the C entry point with y, d_norm, dx
                and d_beta each inside a sentinel-filled arena of exactly its extent (the kernels aim their dropped stores at
                offset 2^31 of a descriptor of M * C * 2 bytes) -- guards intact, every element written, the two results
                bit-equal, d_beta too (its terms are exact).
  geometry      sc2_gdn1_rows_units / sc2_gdn1_rows_workgroups equal ref_gdn_rows.launch() for every case: the tile and strip
                geometry restated there is the only constant of this file, and it is the library's own.

Cases (ref_gdn_rows.CASE_IDS, sized by ref_gdn_rows.case_rows(C, name, P); P = the device's CU count, 256 on the MI355X, asked of the
device inside the tests):

  C = 512, 256    M = 1                 127 rows past the end, all flagged zero, none stored
                  133                   a partial second tile on a second workgroup
                  128 P + 1             exactly one workgroup takes a second tile, holding one row
                  128 (2 P + 3) - 17    (C = 256) third trips and a ragged last tile
  C = 96          M = 1                 one live row in one wave
                  33                    a second wave with one row
                  32 * 8 P + 1          one wave takes a second strip of one row
                  32 (16 P + 11) - 5    third trips, ragged

Also: y bit-equal to the tile kernel's EPI_GDN / EPI_IGDN output on these operands; hip.gdn1_backward with gdn_rows on and off
(off: the two sc2_gdn1_bwd_gemm launches, which no other test holds exactly) -- dx, d_beta, d_gamma equal the reference, which pins
which gamma goes in transposed where; the launchers' refusals.
Measured on an MI355X (profiles/r27_gpu_gdn_rows_tests.log): zero mismatches in every output of every case.
"""
import pytest
import torch

import ref_gdn_rows as R
from test_gpu_stream_kernels import _in_arenas, _same_bits

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
_held = {}


def _cus(dev):
    """P, asked of the device inside a test: importing this file must not initialise the GPU (tests/test_00_*_gpu.py start child
    processes first), so the cases are parametrised by name and sized here."""
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _case(S, dev, C, M, kind):
    """The operands (bf16), the fragment packings and the cast reference of a case, on the device; kept across the parametrisations of
    one (C, M)."""
    key = (C, M, kind)
    if key in _held:
        return _held[key]
    if any(k[:2] != (C, M) for k in _held):
        _held.clear()
        torch.cuda.empty_cache()
    c = R.make_case(C, M, kind, _cus(dev))
    d = dict(C=C, M=M, kind=kind, inverse=c['inverse'])
    for k in ('x', 'g'):
        d[k] = c[k].to(BF).to(dev)
        assert torch.equal(d[k].float().cpu(), c[k])
    d['gamma'], d['beta'] = c['gamma'].to(dev), c['beta'].to(dev)
    d['gf'], d['gtf'] = S.hip.pack_weight_fragments(d['gamma']), S.hip.pack_weight_fragments(d['gamma'].t().contiguous())
    ref = R.reference(d['x'], d['g'], d['gamma'], d['beta'], c['inverse'])
    d['want'] = {k: R.cast(ref[k], BF) for k in ('y', 'd_norm', 'dx')}
    d['want']['d_beta'] = R.cast(ref['d_beta'], F32)
    d['want64'] = {k: ref[k] for k in ('dx', 'd_beta', 'd_gamma')} if M <= 133 else None
    d['zeros'] = int((d['x'] == 0).sum())
    del ref
    _held[key] = d
    return d


def _geometry(S, dev, C, M):
    lib = S.hip.lib()
    L = R.launch(C, M, _cus(dev))
    assert lib.sc2_gdn1_rows_units(M, C) == L['units'] and lib.sc2_gdn1_rows_workgroups(M, C) == L['workgroups'], (C, M)
    return L


def test_reported_geometry_is_the_restated_launch_arithmetic(S, dev):
    lib, _P = S.hip.lib(), _cus(dev)
    extra = [(C, m) for C in (256, 512) for m in (127, 128, 129, 128 * _P - 1, 128 * _P, 256 * _P, 256 * _P + 1)]
    extra += [(96, m) for m in (31, 32, 255, 256, 257, 256 * _P - 1, 256 * _P, 512 * _P, 512 * _P + 1)]
    CASES = R.cases(_P)
    for C, M in CASES + tuple(extra):
        L = _geometry(S, dev, C, M)
        print('C {:3d} M {:7d}: {:5d} units on {:3d} workgroups, {} trips, {:3d} rows in the last unit'.format(
            C, M, L['units'], L['workgroups'], L['trips'], L['last_rows']))
    for C in R.CHANNELS:
        top = (R.LIMIT_BYTES - 1) // (2 * C)
        assert lib.sc2_gdn1_rows_units(top, C) == R.launch(C, top, _P)['units'] and lib.sc2_gdn1_rows_workgroups(top, C) == _P
        for f in (lib.sc2_gdn1_rows_units, lib.sc2_gdn1_rows_workgroups):
            assert f(top + 1, C) == 0 and f(0, C) == 0 and f(-5, C) == 0
    for f in (lib.sc2_gdn1_rows_units, lib.sc2_gdn1_rows_workgroups):
        assert f(100, 128) == 0 and f(100, 0) == 0 and f(100, 1024) == 0
    # the tables reach what they are meant to reach on THIS device
    assert sorted({R.launch(C, M, _P)['trips'] for C, M in CASES}) == [1, 2, 3]
    for C in R.CHANNELS:
        L = R.launch(*R.second_trip_case(C, _P), _P)
        assert L['trips'] == 2 and L['last_rows'] == 1 and L['units'] == L['workers'] + 1


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C,name', R.CASE_IDS)
def test_rows_kernels_equal_the_reference(S, dev, C, name, kind, direction):
    hip, lib = S.hip, S.hip.lib()
    M = R.case_rows(C, name, _cus(dev))
    c = _case(S, dev, C, M, kind)
    L = _geometry(S, dev, C, M)
    p, st, inv = hip._ptr, hip._stream(), int(c['inverse'])
    unit = R.UNIT_ROWS[C]
    tag = 'C {} M {} {} {} [{} units, {} workgroups, {} trips, {} rows last; {} zeros of x]'.format(
        C, M, kind, direction, L['units'], L['workgroups'], L['trips'], L['last_rows'], c['zeros'])
    if direction == 'fwd':
        y = hip.gdn1_rows_fwd(c['x'], c['gf'], c['beta'], c['inverse'])
        assert y.shape == (M, C) and y.dtype == BF
        y2, = _in_arenas(dev, [(M * C, BF)], lambda o: lib.sc2_gdn1_rows_fwd(p(c['x']), p(c['gf']), p(c['beta']), o, M, C, inv, st), tag)
        assert _same_bits(y, y2), tag + ': two launches differ'
        R.assert_same(y, c['want']['y'], tag + ' y', unit)
        print(tag + ': mismatches y 0')
        return
    d_norm, dx, d_beta = hip.gdn1_rows_bwd(c['x'], c['g'], c['gf'], c['gtf'], c['beta'], c['inverse'], want_d_beta=True)
    assert d_norm.shape == dx.shape == (M, C) and d_norm.dtype == dx.dtype == BF and d_beta.shape == (C,) and d_beta.dtype == F32
    a_norm, a_dx, a_beta = _in_arenas(
        dev, [(M * C, BF), (M * C, BF), (C, F32)],
        lambda o1, o2, o3: lib.sc2_gdn1_rows_bwd(p(c['x']), p(c['g']), p(c['gf']), p(c['gtf']), p(c['beta']), o1, o2, o3, M, C, inv, st), tag)
    assert _same_bits(d_norm, a_norm) and _same_bits(dx, a_dx) and _same_bits(d_beta, a_beta), tag + ': two launches differ'
    R.assert_same(d_norm, c['want']['d_norm'], tag + ' d_norm', unit)
    R.assert_same(dx, c['want']['dx'], tag + ' dx', unit)
    R.assert_same(d_beta, c['want']['d_beta'], tag + ' d_beta')
    print(tag + ': mismatches d_norm 0 dx 0 d_beta 0')


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C,name', [(C, name) for C, name in R.CASE_IDS if name != 'third_trip'])
def test_forward_equals_the_tile_kernels_fused_epilogue(S, dev, C, name, kind):
    """The equality of test_gdn512_rows on the new operands: the tile kernel's EPI_GDN / EPI_IGDN forms the same products."""
    hip = S.hip
    M = R.case_rows(C, name, _cus(dev))
    c = _case(S, dev, C, M, kind)
    y = hip.gdn1_rows_fwd(c['x'], c['gf'], c['beta'], c['inverse'])
    x4 = c['x'].view(1, 1, M, C)
    y_tile = hip.conv2d_fwd(x4, hip.pack_conv_weight(c['gamma'].reshape(C, C, 1, 1)), C, 1, 1, 1, 0, a_op=hip.AOP_ABS,
                            epilogue=hip.EPI_IGDN if c['inverse'] else hip.EPI_GDN, ep_x=x4, ep_beta=c['beta'])
    assert _same_bits(y, y_tile.reshape(M, C))
    R.assert_same(y_tile.reshape(M, C), c['want']['y'], 'tile kernel y', R.UNIT_ROWS[C])


@pytest.mark.parametrize('rows', [True, False], ids=['rows', 'two_gemms'])
@pytest.mark.parametrize('kind', ['narrow', 'div'])
@pytest.mark.parametrize('C,name', R.SMALL_IDS)
def test_gdn1_backward_composition_is_exact(S, dev, C, name, kind, rows):
    """hip.gdn1_backward with host_policy.gdn_rows on (one launch + the weight gradient) and off (the two sc2_gdn1_bwd_gemm
    launches, a column sum, the weight gradient): dx, d_beta, d_gamma equal the reference.  'narrow' and 'div': the two-launch form
    hands d_norm AND the direct term dd on as bf16, and both are bf16-exact there (ref_gdn_rows, check_exactness)."""
    hip = S.hip
    M = R.case_rows(C, name, _cus(dev))
    c = _case(S, dev, C, M, kind)
    before = bool(hip.host_policy.gdn_rows)
    hip.configure(gdn_rows=rows)
    try:
        dx, d_beta, d_gamma = hip.gdn1_backward(c['g'].view(1, 1, M, C), c['x'].view(1, 1, M, C), c['beta'], c['gamma'], c['inverse'])
        torch.cuda.synchronize()
    finally:
        hip.configure(gdn_rows=before)
    assert dx.dtype == BF and d_beta.dtype == F32 and d_gamma.dtype == F32 and tuple(d_gamma.shape) == (C, C)
    tag = 'gdn1_backward C {} M {} {} gdn_rows {}'.format(C, M, kind, rows)
    R.assert_same(dx.reshape(M, C), R.cast(c['want64']['dx'], BF), tag + ' dx', R.UNIT_ROWS[C])
    R.assert_same(d_beta, R.cast(c['want64']['d_beta'], F32), tag + ' d_beta')
    R.assert_same(d_gamma.contiguous(), R.cast(c['want64']['d_gamma'], F32), tag + ' d_gamma')


def test_refusals(S, dev):
    """What the launchers refuse -- C outside {96, 256, 512} and tensors of 0x7FF00000 bytes or more: SC2_ERR_UNSUPPORTED; null
    pointers: SC2_ERR_INVALID_ARG -- and nothing is written, d_beta not zeroed either."""
    hip, lib = S.hip, S.hip.lib()
    p, st = hip._ptr, hip._stream()
    INVALID, UNSUPPORTED = -1, -2
    b = torch.ones(512 * 4, dtype=BF, device=dev)
    frag = torch.ones(512 * 512, dtype=BF, device=dev)
    beta = torch.ones(512, dtype=F32, device=dev)
    o1, o2 = torch.full((4096,), 3.0, dtype=BF, device=dev), torch.full((4096,), 3.0, dtype=BF, device=dev)
    of = torch.full((512,), 3.0, dtype=F32, device=dev)

    def fwd(x=p(b), gf=p(frag), be=p(beta), y=p(o1), M=4, C=512, inverse=1):
        return lib.sc2_gdn1_rows_fwd(x, gf, be, y, M, C, inverse, st)

    def bwd(x=p(b), g=p(b), gf=p(frag), gtf=p(frag), be=p(beta), dn=p(o1), dx=p(o2), db=p(of), M=4, C=512, inverse=1):
        return lib.sc2_gdn1_rows_bwd(x, g, gf, gtf, be, dn, dx, db, M, C, inverse, st)

    got, want = [], []
    for C in (0, 8, 48, 128, 192, 384, 1024, -96):
        got += [fwd(C=C), bwd(C=C), lib.sc2_gdn1_rows_supported(C)]
        want += [UNSUPPORTED, UNSUPPORTED, 0]
    for C in R.CHANNELS:
        assert lib.sc2_gdn1_rows_supported(C) == 1
        too_many = (R.LIMIT_BYTES + 2 * C - 1) // (2 * C)                          # the first M with M * C * 2 >= 0x7FF00000
        assert (too_many - 1) * 2 * C < R.LIMIT_BYTES <= too_many * 2 * C
        for M in (too_many, 1 << 40, 0, -4):
            for inverse in (0, 1):
                got += [fwd(M=M, C=C, inverse=inverse), bwd(M=M, C=C, inverse=inverse)]
                want += [UNSUPPORTED, UNSUPPORTED]
        for name in ('x', 'gf', 'be', 'y'):
            got.append(fwd(C=C, **{name: None}))
            want.append(INVALID)
        for name in ('x', 'g', 'gf', 'gtf', 'be', 'dn', 'dx'):
            got.append(bwd(C=C, **{name: None}))
            want.append(INVALID)
    torch.cuda.synchronize()
    assert got == want, [(i, a, b_) for i, (a, b_) in enumerate(zip(got, want)) if a != b_]
    assert bool((o1 == 3.0).all()) and bool((o2 == 3.0).all()) and bool((of == 3.0).all())
    x = torch.ones((4, 128), dtype=BF, device=dev)
    assert not hip.gdn1_rows_supported(x, 128) and hip.gdn1_rows_supported(torch.ones((4, 96), dtype=BF, device=dev), 96)
