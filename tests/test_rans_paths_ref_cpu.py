"""tests/ref_rans_paths.py against the oracle and against itself (no GPU): the case table reaches every decode-side kernel by the
restated dispatch, each case's stated reason holds on the tables as built, and every expected value stands on the oracle alone."""
import numpy as np
import pytest
import torch

from oracle import rans as oracle_rans

import ref_rans_paths as ref

LAUNCHED = [c for c in ref.CASES if c.launch]


def _plan(c):
    n_cdfs, stride = ref.case_shape(c)
    return ref.plan(c.explicit, c.index_div, c.S, c.n_sym, n_cdfs, stride, fused_dq=c.fused, policy=c.policy)


def test_cases_name_every_decode_kernel():
    plans = {c.name: _plan(c) for c in ref.CASES}
    launched = {c.name: plans[c.name] for c in LAUNCHED}
    assert {p[0] for p in launched.values()} == {'lut8', 'lut-u8', 'lut-u16', 'ragged2', 'ragged-8bit', 'ragged-5bit', 'generic-lds',
                                                 'generic-global'}
    assert {p[2] for p in launched.values()} == {'none', 'transpose', 'dq-reg', 'dq-lds'}
    assert {p[1] for p in launched.values() if p[0] == 'ragged2'} == {1, 2, 4, 8}
    assert {c.C for c in LAUNCHED if launched[c.name][2] == 'dq-reg'} == {8, 16, 24, 32}
    assert {c.C for c in LAUNCHED if launched[c.name][2] == 'dq-lds'} == {8, 24, 32, 40, 48, 56, 64}
    # every fused form behind every implicit-index decoder
    assert {(p[0], p[2]) for p in launched.values() if p[2].startswith('dq')} >= {('lut-u8', 'dq-reg'), ('lut-u16', 'dq-reg'), ('lut8', 'dq-reg'),
                                                                                   ('lut-u8', 'dq-lds'), ('lut8', 'dq-lds')}
    # each case reaches what its name says
    for name, (path, waves, finish) in plans.items():
        if name.startswith('dq-reg') or name.startswith('dq-lds'):
            assert finish == name[:6], name
            assert path == (name.split('behind ')[1] if 'behind' in name else 'lut-u8'), name
        elif name.startswith('lut8'):
            assert finish == 'transpose' and (path == 'lut8') == ('fall' not in name), name
        elif name.startswith('ragged2'):
            assert path == 'ragged2' and finish == 'transpose', name
            if ' w' in name:
                assert waves == int(name.split(' w')[1].split(' ')[0]), name
        elif name.startswith('ragged8'):
            assert (path, waves, finish) == ('ragged-8bit', 1, 'transpose'), name
        elif name.startswith('ragged5'):
            assert (path, waves, finish) == ('ragged-5bit', 1, 'transpose'), name
        else:
            assert (path + ' ').startswith(name.split(' ')[0] + ' ') and finish == 'none', name
    assert plans['lut8 stride 258 falls back'][0] == 'lut-u16' and plans['lut8 1025 rows fall back'][0] == 'lut-u8'
    assert plans['ragged2 default S1024'][1] == 2 and plans['ragged2 default S70'][1] == 1
    # the launch bounds of the table: at most 130 streams of at most 400 symbols, the 1 024-stream case apart (fused cases: C HW symbols)
    for c in LAUNCHED:
        assert c.S <= 130 or c.name == 'ragged2 default S1024', c.name
        assert c.n_sym <= 400 or c.fused, c.name
        assert not c.fused or (c.HW <= 33 and c.S <= 70), c.name
    # the damaged-stream runs: each newly reached serial kernel once, and the fused pass behind lut-u8
    assert sorted((plans[c.name][0], plans[c.name][1], plans[c.name][2]) for c in ref.CASES if c.damage) == sorted([
        ('lut8', 1, 'transpose'), ('ragged2', 2, 'transpose'), ('ragged-8bit', 1, 'transpose'), ('generic-global', 1, 'none'),
        ('lut-u8', 1, 'dq-reg')])
    assert all(c.S >= 65 for c in ref.CASES if c.damage)


def test_plan_thresholds():
    """the dispatch on both sides of each constant"""
    P = ref.plan
    assert P(False, 10, 4, 40, 4, 257)[0] == 'lut-u8' and P(False, 10, 4, 40, 4, 258)[0] == 'lut-u16'
    assert P(False, 10, 4, 40, 4, 4096)[0] == 'lut-u16' and P(False, 10, 4, 40, 2, 4097)[0] == 'generic-lds'
    assert P(False, 10, 4, 40, 3, 4096, policy={'rans_lut8': 1})[0] == 'lut-u16'
    assert P(False, 1, 4, 1024, 1024, 12, policy={'rans_lut8': 1})[0] == 'lut8'
    assert P(True, 0, 4, 40, 64, 192)[0] == 'generic-lds' and P(True, 0, 4, 40, 64, 193)[0] == 'ragged2'
    assert P(True, 0, 4, 40, 65, 193)[0] == 'ragged-5bit' and P(True, 0, 4, 40, 256, 49)[0] == 'ragged-5bit'
    assert P(True, 0, 4, 40, 257, 49)[0] == 'generic-global'
    assert P(True, 0, 1023, 40, 64, 193)[1] == 1 and P(True, 0, 1024, 40, 64, 193)[1] == 2
    assert [P(True, 0, 4, 40, 64, 193, policy={'rans_ragged2_waves': v})[1] for v in (1, 2, 3, 4, 5, 8, 9)] == [1, 2, 4, 4, 8, 8, 8]
    for C in range(8, 72, 8):
        assert P(False, 5, 4, 5 * C, C, 30, fused_dq=True)[2] == ('dq-reg' if C <= 32 else 'dq-lds')
        assert P(False, 5, 4, 5 * C, C, 30, fused_dq=True, policy={'rans_dq_lds': 1})[2] == 'dq-lds'
    assert P(False, 5, 4, 0, 8, 30, fused_dq=True)[2] == 'none' and P(True, 0, 4, 0, 64, 193)[2] == 'none'


def test_stated_reasons_hold_on_the_built_tables():
    for c in LAUNCHED:
        b = ref.build(c)
        n_cdfs, stride = b.cdfs.shape
        assert len(set(b.offs.tolist())) == n_cdfs, c.name                  # distinct offsets per row
        assert (b.sizes >= 5).all() and int(b.sizes.max()) == stride, c.name
        for r in range(n_cdfs):
            row = b.cdfs[r, :b.sizes[r]]
            assert row[0] == 0 and row[-1] == 65536 and (np.diff(row) > 0).all(), c.name
        # escapes on both sides of the range, regular symbols between them
        v = b.sym.astype(np.int64) - b.offs[b.row_of]
        if c.S * c.n_sym >= 2000:
            assert (v < 0).any() and (v >= b.sizes[b.row_of] - 2).any(), c.name
        assert ((v >= 0) & (v < b.sizes[b.row_of] - 2)).mean() > 0.5 or c.S * c.n_sym < 50, c.name
        if c.explicit:
            assert n_cdfs * stride > ref.LDS_ENTRY_LIMIT, c.name               # more than 12 288 entries
            assert b.idx.min() == 0 and b.idx.max() == n_cdfs - 1, c.name
        if c.fused:
            assert b.medians[0] == 0.0 and len(set(b.medians.tolist())) == n_cdfs, c.name
            assert b.sizes[0] - 2 + b.offs[0] <= 259, c.name                   # the ties are escapes of channel 0
            pos = ref.tie_positions(c.HW)
            for k, p in enumerate(pos):
                assert (b.sym[:, p] == ref.TIES[k]).all(), c.name
            assert (b.sym[:, 0] == 259).all(), c.name                           # ties present in every fused case
            if c.HW >= 4:
                assert len(pos) == 4 and pos[-1] == c.HW - 1, c.name
            want = ref.dequantize_ref(b.sym, b.medians, c.HW)
            assert want[0, 0, 0].item() == 260.0                                # 259 rounds to even, not down to 258
    # in LDS / not in LDS, by the packed sizes the kernels compare with their capacity
    fits2 = {c.name: ref.ragged2_entries(ref.build(c).sizes) <= ref.K_RAGGED2_CAP for c in LAUNCHED if c.name.startswith('ragged2')}
    assert all(fits2[n] == ('not in LDS' not in n) for n in fits2) and not all(fits2.values()) and any(fits2.values())
    for name, fits in (('ragged8 in LDS', True), ('ragged8 not in LDS', False), ('ragged5 in LDS', True), ('ragged5 not in LDS', False)):
        assert (ref.ragged_entries(ref.build(ref.CASE_BY_NAME[name]).sizes) <= ref.K_RAGGED_CAP) == fits, name
    assert ref.build(ref.CASE_BY_NAME['ragged8 in LDS']).cdfs.shape == (40, 600)
    assert ref.build(ref.CASE_BY_NAME['ragged8 not in LDS']).cdfs.shape == (64, 2400)
    assert 65 <= ref.build(ref.CASE_BY_NAME['ragged5 not in LDS']).cdfs.shape[0] <= 256
    assert ref.build(ref.CASE_BY_NAME['generic-global 300 rows']).cdfs.shape == (300, 42)
    assert ref.build(ref.CASE_BY_NAME['generic-global stride 4100']).cdfs.shape == (4, 4100)
    assert ref.build(ref.CASE_BY_NAME['generic-lds stride 4100']).cdfs.shape == (2, 4100)
    assert 300 in ref.build(ref.CASE_BY_NAME['dq-reg C24 behind lut-u16']).sizes
    # the lut8 table: a row of 257 entries whose last symbol is reachable, multi buckets, and symbols drawn inside them
    for S in (1, 64, 65):
        c = ref.CASE_BY_NAME['lut8 multi S{}'.format(S)]
        b = ref.build(c)
        assert b.sizes[1] == 257 and b.cdfs.shape[1] == 257
        multi = ref.lut8_buckets(b.cdfs[1], 257)
        assert int(multi.sum()) >= 20
        assert not ref.lut8_buckets(b.cdfs[0], int(b.sizes[0]))[:8].all()          # (not everything is multi)
        row1 = b.sym[:, 126:252]
        assert ref.lut8_symbols_in_multi(b.cdfs[1], 257, int(b.offs[1]), row1) >= 50
        v1 = row1.astype(np.int64) - b.offs[1]
        assert ((v1 < 0) | (v1 >= 255)).any()              # symbol index 255 (the row's escape symbol) is coded
        assert (v1 == 254).any() or S == 1                  # ... and so is the last regular one
        assert c.index_div % 8 == 6
    assert ref.CASE_BY_NAME['lut8 div5'].index_div < 8
    c = ref.CASE_BY_NAME['lut8 div8 partial']
    assert c.index_div == 8 and c.n_sym % 8 == 3


def test_lut8_bucket_rule_on_a_hand_table():
    """cdf 0 | 3 | 5 | 6 | 20 | 65536: bucket 0 (values 0 .. 7) starts in symbol 0, which ends at 3, its successor at 5 < 8: multi;
    bucket 1 (8 .. 15) lies inside symbol 3; bucket 2 (16 .. 23) starts in symbol 3, which ends at 20, its successor at 65536"""
    cdf = [0, 3, 5, 6, 20, 65536]
    m = ref.lut8_buckets(cdf, 6)
    assert m[0] and not m[1:].any()
    assert ref.lut8_symbols_in_multi(cdf, 6, -2, [-2, -1, 0, 1, 2, 99]) == 3      # symbols 0, 1, 2 lie inside bucket 0; 3 does not


def test_oracle_decodes_its_own_bytes_for_every_stream():
    for c in LAUNCHED:
        b = ref.build(c)
        assert len(b.streams) == c.S
        for i in range(c.S):
            got = oracle_rans.decode_with_indexes(b.streams[i], b.row_of[i], b.cdfs, b.sizes, b.offs)
            assert np.array_equal(got, b.sym[i]), (c.name, i)


@pytest.mark.parametrize('name', ['dq-reg C24 HW23 S70', 'dq-lds C48 HW33 S70'])
def test_dequantize_ref_is_the_oracles_dequantize(R, name):
    c = ref.CASE_BY_NAME[name]
    b = ref.build(c)
    sym = torch.from_numpy(np.array(b.sym)).reshape(c.S, c.C, c.HW, 1)
    y = R.EntropyBottleneck.dequantize(sym, torch.from_numpy(np.array(b.medians)).reshape(1, c.C, 1, 1))
    assert y.dtype == torch.float32
    want = y.permute(0, 2, 3, 1).reshape(c.S, c.HW, c.C).to(torch.bfloat16)
    got = ref.dequantize_ref(b.sym, b.medians, c.HW)
    assert got.shape == want.shape and torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the ties of channel 0 round to even
    pos = ref.tie_positions(c.HW)
    assert [got[0, p, 0].item() for p in pos] == [260.0, 260.0, -260.0, 70144.0]


def test_packing_round_trips():
    for name in ('ragged2 w2 S70', 'dq-reg C8 HW1 S1', 'lut8 multi S65'):
        b = ref.build(ref.CASE_BY_NAME[name])
        for stride in (None, 4096):
            buf, off, nb = ref.pack_streams(b.streams, stride)
            assert buf.dtype == np.uint8 and buf.shape[1] % 4 == 0 and buf.shape[1] >= 8
            assert (off % 4 == 0).all() and (off + nb == buf.shape[1]).all()
            assert ref.unpack_streams(buf, off, nb) == b.streams
        bad, which = ref.damage(b.streams) if len(b.streams) >= 65 else (None, None)
        if bad:
            buf, off, nb = ref.pack_streams(bad, 4096)
            assert ref.unpack_streams(buf, off, nb) == bad and which == [3, 9, 64]
            assert set(bad[3]) == {255} and len(bad[3]) == len(b.streams[3]) and bad[9] == b.streams[9][:16] and len(bad[64]) == 8
            assert all(bad[i] == b.streams[i] for i in range(len(bad)) if i not in which)


def test_library_reports_the_restated_dispatch(S):
    """sc2_rans_decode_path is host arithmetic over the policy: the library's decision equals plan() for every case, under the case's
    policy, without a device (tests/test_gpu_rans_paths.py asserts the same in front of each launch)."""
    hip = S.hip
    before = hip.get_policy()
    saved = {f: getattr(before, f) for f in ref.DEFAULT_POLICY}
    assert saved == ref.DEFAULT_POLICY
    try:
        for c in ref.CASES:
            hip.configure(**dict(saved, **c.policy))
            n_cdfs, stride = ref.case_shape(c)
            assert hip.rans_decode_path(c.explicit, c.index_div, c.S, c.n_sym, n_cdfs, stride, fused_dq=c.fused) == _plan(c), c.name
    finally:
        hip.configure(**saved)
    assert sorted(hip.RANS_DEC_PATHS.values()) == sorted(['lut8', 'lut-u8', 'lut-u16', 'ragged2', 'ragged-8bit', 'ragged-5bit', 'generic-lds',
                                                          'generic-global'])


def test_decode_path_refuses_sizes_no_call_takes(S):
    hip = S.hip
    assert hip.lib().sc2_rans_decode_path(0, 0, 4, 40, 4, 30, 0, None, None) == 0       # implicit indexes without index_div
    assert hip.lib().sc2_rans_decode_path(1, 0, 0, 40, 4, 30, 0, None, None) == 0
    assert hip.lib().sc2_rans_decode_path(1, 0, 4, 40, 4, 2, 0, None, None) == 0
    with pytest.raises(hip.Sc2Error):
        hip.rans_decode_path(False, 0, 4, 40, 4, 30)
