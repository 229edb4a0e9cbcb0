"""References and the case table of the range-decoder path tests (CPU only: numpy, torch on the host, the C oracle; no GPU import).

tests/test_rans_paths_ref_cpu.py checks this file against the oracle and against itself; tests/test_gpu_rans_paths.py runs every
case of CASES on the device.  Everything a case expects stands on the oracle (oracle/rans.py): its tables come from
pmf_to_quantized_cdf, its streams from encode_with_indexes, and the symbols those bytes decode to are the case's own.

  plan(...)            the decode dispatch of csrc/rans.hip (decode_plan) restated from its constants
  dequantize_ref(...)  the fused pass's expected value: bf16(f32(symbol + median)) as NHWC
  lut8_buckets(...)    the bucket rule of rans_build_dec_table_kernel: which 8-wide buckets hold two boundaries ("multi")
  pack_streams(...)    byte strings -> the end-aligned [n_streams, stride] rows + off / nb of sc2_rans_decode_batch
  CASES / build(case)  the smallest shapes that reach each decoder, and their tables, symbols, indexes and oracle streams

Which case launches which kernel (kernel names of csrc/rans.hip; `path`, `waves`, `finish` are what plan() returns):

  rans_dec_finish_dq_reg_kernel<8 / 16 / 24 / 32>   finish dq-reg   cases 'dq-reg C<C> ...'
  rans_dec_finish_dq_kernel                         finish dq-lds   cases 'dq-lds C<C> ...'
  rans_build_dec_table_kernel, rans_dec_lut8_kernel path lut8       cases 'lut8 ...', 'dq-reg C24 behind lut8', 'dq-lds C48 behind lut8'
  rans_dec_ragged2_kernel<2 / 4 / 8>                path ragged2, waves 2 / 4 / 8   cases 'ragged2 w<waves> ...', 'ragged2 default S1024'
  rans_dec_ragged_kernel<8>                         path ragged-8bit cases 'ragged8 ...'
  rans_dec_ragged_kernel<5> (global-table fallback) path ragged-5bit case 'ragged5 not in LDS'
  rans_dec_generic_kernel<false>                    path generic-global  cases 'generic-global ...'
and, already reached elsewhere in the suite but listed so that the table names every decode-side kernel: rans_dec_lut_kernel
<uint8_t> / <uint16_t> (lut-u8 / lut-u16), rans_dec_ragged2_kernel<1>, rans_dec_ragged_kernel<5> in LDS,
rans_dec_generic_kernel<true> (generic-lds), rans_dec_finish_kernel and rans_transpose_in_kernel (finish transpose).
"""
import collections
import zlib

import numpy as np
import torch

from oracle import rans as oracle_rans

# ---------------------------------------------------------------------------------------------- the dispatch, restated
K_MAX_ROW_LDS = 4096        # longest CDF row of the LUT decoders
LDS_ENTRY_LIMIT = 12288     # rectangular table entries the generic decoder keeps in LDS
K_RAGGED2_ROWS = 64
K_RAGGED_ROWS = 256
K_RAGGED2_CAP = 45056       # packed u16 entries incl. 8 sentinels per row
K_RAGGED_CAP = 61440
K_PROBE = 8                 # sentinels behind a row of the four-lane decoder
LUT8_MAX_STRIDE, LUT8_MAX_ROWS = 257, 1024
DQ_REG_CHANNELS = (8, 16, 24, 32)
RAGGED2_WIDE_STREAMS = 1024  # default policy: two waves per workgroup from here
DEFAULT_POLICY = {'rans_lut8': 0, 'rans_dq_lds': 0, 'rans_ragged2': 1, 'rans_ragged2_waves': 0}


def plan(explicit_indexes, index_div, n_streams, n_sym, n_cdfs, cdf_stride, fused_dq=False, policy=None):
    """-> (serial kernel, waves per workgroup, finishing pass), by the names of hip.RANS_DEC_PATHS / RANS_DEC_FINISHES."""
    pol = dict(DEFAULT_POLICY)
    pol.update(policy or {})
    n_entries = n_cdfs * cdf_stride
    if not explicit_indexes and cdf_stride <= K_MAX_ROW_LDS:
        if pol['rans_lut8'] and cdf_stride <= LUT8_MAX_STRIDE and n_cdfs <= LUT8_MAX_ROWS:
            path = 'lut8'
        else:
            path = 'lut-u8' if cdf_stride <= 257 else 'lut-u16'
        if n_sym == 0:
            finish = 'none'
        elif not fused_dq:
            finish = 'transpose'
        else:
            finish = 'dq-reg' if n_cdfs in DQ_REG_CHANNELS and not pol['rans_dq_lds'] else 'dq-lds'
        return path, 1, finish
    if explicit_indexes and n_entries > LDS_ENTRY_LIMIT and n_cdfs <= K_RAGGED_ROWS:
        finish = 'transpose' if n_sym > 0 else 'none'
        if n_cdfs <= K_RAGGED2_ROWS and pol['rans_ragged2']:
            v = pol['rans_ragged2_waves']
            waves = (2 if n_streams >= RAGGED2_WIDE_STREAMS else 1) if v <= 0 else 1 if v <= 1 else 2 if v <= 2 else 4 if v <= 4 else 8
            return 'ragged2', waves, finish
        return ('ragged-8bit' if n_cdfs <= 64 else 'ragged-5bit'), 1, finish
    return ('generic-lds' if n_entries <= LDS_ENTRY_LIMIT else 'generic-global'), 1, 'none'


def ragged2_entries(sizes):
    """u16 entries the four-lane decoder packs: every row with its 8 sentinels (in LDS iff <= K_RAGGED2_CAP)"""
    return int(sum(int(s) + K_PROBE for s in sizes))


def ragged_entries(sizes):
    """u16 entries the one-lane ragged decoder packs (in LDS iff <= K_RAGGED_CAP)"""
    return int(sum(int(s) for s in sizes))


# ---------------------------------------------------------------------------------------------- dequantise reference
def dequantize_ref(sym, medians, HW):
    """sym: int [S, C * HW] (position c * HW + pix), medians: f32 [C] -> bf16 [S, HW, C]: the symbol as float64 plus the median as
    float64, rounded to float32, then to bfloat16 (torch's cast: round to nearest even).  |symbol| < 2^24, so (float)symbol is exact."""
    sym = np.asarray(sym)
    medians = np.array(medians, dtype=np.float32)
    S, C = sym.shape[0], medians.size
    assert sym.shape[1] == C * HW and np.abs(sym).max() < 1 << 24
    v = torch.from_numpy(sym.astype(np.int64)).double().reshape(S, C, HW) + torch.from_numpy(medians).double().reshape(1, C, 1)
    return v.to(torch.float32).permute(0, 2, 1).contiguous().to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- lut8 bucket rule
def lut8_buckets(cdf, size):
    """rans_build_dec_table_kernel per bucket b of eight cumulative frequencies, restated: A = the last symbol whose start is <=
    8 b, B = A + 1; the bucket is `multi` iff B ends inside it too (and is not the row's last boundary, 65536).
    -> bool [8192]."""
    cdf = [int(v) for v in cdf[:size]]
    multi = np.zeros(8192, dtype=bool)
    A = 0
    for b in range(8192):
        cf0 = b * 8
        while A + 1 <= size - 2 and cdf[A + 1] <= cf0:
            A += 1
        end_a = cdf[A + 1]
        end_b = cdf[A + 2] if A + 2 <= size - 1 else end_a
        multi[b] = end_b < cf0 + 8 and end_b < 65536
    return multi


def lut8_symbols_in_multi(cdf, size, offset, symbols):
    """how many of `symbols` (of this row) are CERTAIN to be decoded from a multi bucket: regular symbols whose every cumulative
    frequency [start, end) lies in one"""
    multi = lut8_buckets(cdf, size)
    certain = np.zeros(size - 1, dtype=bool)
    for k in range(size - 2):      # regular symbols (size - 2 is the escape symbol)
        certain[k] = all(multi[c >> 3] for c in range(int(cdf[k]), int(cdf[k + 1])))
    v = np.asarray(symbols, dtype=np.int64) - offset
    ok = (v >= 0) & (v < size - 2)
    return int(certain[v[ok]].sum())


# ---------------------------------------------------------------------------------------------- stream packing
def pack_streams(streams, stride=None):
    """Byte strings -> (buf u8 [n, stride], off i32 [n], nb i32 [n]): stream i occupies buf[i, off[i]:off[i] + nb[i]], END-aligned
    in its row (include/sc2_bottleneck.h: rANS emits its words back to front), off % 4 == 0, stride % 4 == 0, stride >= 8."""
    longest = max(len(s) for s in streams)
    if stride is None:
        stride = max(8, (longest + 3) // 4 * 4)
    assert stride % 4 == 0 and stride >= 8 and stride >= longest
    buf = np.zeros((len(streams), stride), dtype=np.uint8)
    off = np.zeros(len(streams), dtype=np.int32)
    nb = np.zeros(len(streams), dtype=np.int32)
    for i, s in enumerate(streams):
        assert len(s) % 4 == 0
        off[i], nb[i] = stride - len(s), len(s)
        buf[i, stride - len(s):] = np.frombuffer(s, dtype=np.uint8)
    return buf, off, nb


def unpack_streams(buf, off, nb):
    return [buf[i, off[i]:off[i] + nb[i]].tobytes() for i in range(buf.shape[0])]


# ---------------------------------------------------------------------------------------------- tables and symbols
TIES = (259, 261, -259, 70000)     # channel 0 (median 0.0): 259 and 261 are round-to-even ties of bf16 (-> 260), a truncating store gives 258


def _cdf_of(pmf):
    return [int(v) for v in oracle_rans.pmf_to_quantized_cdf(np.asarray(pmf, dtype=np.float32))]


def make_tables(rng, lengths, pmfs=None):
    """lengths: pmf length per row (the row has length + 1 entries; its last symbol is the escape symbol) -> cdfs i32 [n, stride],
    sizes, offsets (distinct per row), medians f32 (row 0: 0.0, the others N(0, 1), distinct)."""
    rows, sizes, offs = [], [], []
    for r, n in enumerate(lengths):
        if pmfs is not None and pmfs.get(r) is not None:
            p = np.asarray(pmfs[r], dtype=np.float32)
            assert p.size == n
        else:
            p = rng.rand(n).astype(np.float32) ** 2 + 1e-4
        p = p / p.sum()
        cdf = _cdf_of(p)
        assert len(cdf) == n + 1 and cdf[0] == 0 and cdf[-1] == 65536
        rows.append(cdf)
        sizes.append(n + 1)
        o = -(n // 2)
        while o in offs:
            o -= 1
        offs.append(o)
    stride = max(sizes)
    cdfs = np.zeros((len(rows), stride), dtype=np.int32)
    for r, c in enumerate(rows):
        cdfs[r, :len(c)] = c
    med = rng.randn(len(rows)).astype(np.float32)
    med[0] = 0.0
    return cdfs, np.array(sizes, dtype=np.int32), np.array(offs, dtype=np.int32), med


def draw_symbols(rng, row_of, sizes, offs, escapes=0.04):
    """row_of: int [S, n_sym] CDF row per symbol -> symbols uniform over each row's regular range [offset, offset + size - 2), a
    few percent outside it on both sides (escapes, up to 40 away)."""
    nreg = (sizes[row_of] - 2).astype(np.int64)
    v = (rng.rand(*row_of.shape) * nreg).astype(np.int64)
    u = rng.rand(*row_of.shape)
    d = rng.randint(1, 41, size=row_of.shape)
    v = np.where(u < escapes / 2, -d, v)
    v = np.where(u > 1 - escapes / 2, nreg - 1 + d, v)
    return (v + offs[row_of]).astype(np.int32)


def tie_positions(HW):
    """pixels of channel 0 that carry TIES: spread over the plane, the last pixel among them; fewer where the plane is smaller"""
    return [0, HW // 3, 2 * HW // 3, HW - 1] if HW >= 4 else list(range(HW))


def multi_row_pmf(rng):
    """256 symbols: a head of 60 with real mass, then runs of 13 symbols of (quantised) frequency 1 separated by one heavier
    symbol -- the far tail of a trained table, where eight cumulative frequencies hold several boundaries"""
    p = np.full(256, 1e-9, dtype=np.float64)
    p[:60] = rng.rand(60) ** 2 + 0.01
    p[73::14] = 0.002
    return p / p.sum()


Case = collections.namedtuple('Case', 'name policy explicit index_div S n_sym fused C HW table launch damage why')


def _case(name, S, n_sym, table, policy=None, explicit=False, index_div=0, fused=False, C=0, HW=0, launch=True, damage=False, why=''):
    return Case(name, dict(policy or {}), explicit, index_div, S, n_sym, fused, C, HW, table, launch, damage, why)


def _cases():
    out = []
    # ---- fused decode + dequantise (implicit indexes, index_div = HW, n_sym = C HW)
    for C in (8, 16, 24, 32):
        for HW, S, why in ((1, 1, 'three waves leave at once, the fourth has no second pixel'),
                           (9, 65, 'a second workgroup of one pixel, a second stream block of one stream'),
                           (23, 70, 'odd HW: the last wave has no second pixel')):
            out.append(_case('dq-reg C{} HW{} S{}'.format(C, HW, S), S, C * HW, ('eb', C), index_div=HW, fused=True, C=C, HW=HW,
                             damage=(C, HW) == (24, 23), why=why))
    for C, pol in ((40, {}), (48, {}), (56, {}), (64, {}), (8, {'rans_dq_lds': 1}), (24, {'rans_dq_lds': 1}), (32, {'rans_dq_lds': 1})):
        for HW, S, why in ((1, 1, 'a block of one pixel'), (16, 64, 'exact blocks'), (17, 65, 'a second block of one pixel / one stream'),
                           (33, 70, 'two whole pixel blocks and a ragged one')):
            out.append(_case('dq-lds C{} HW{} S{}'.format(C, HW, S), S, C * HW, ('eb', C), policy=pol, index_div=HW, fused=True, C=C, HW=HW,
                             why=why))
    # behind each implicit-index decoder ('dq-reg C24 HW23 S70' above is the one behind lut-u8, the default)
    out.append(_case('dq-reg C24 behind lut-u16', 70, 24 * 23, ('eb-wide', 24), index_div=23, fused=True, C=24, HW=23, why='one row of 300 entries'))
    out.append(_case('dq-reg C24 behind lut8', 70, 24 * 23, ('eb', 24), policy={'rans_lut8': 1}, index_div=23, fused=True, C=24, HW=23))
    out.append(_case('dq-lds C48 behind lut8', 70, 48 * 23, ('eb', 48), policy={'rans_lut8': 1}, index_div=23, fused=True, C=48, HW=23))
    # ---- lut8, plain decode (126 = 15 * 8 + 6: every row ends in a ragged 6-symbol tail)
    for S in (1, 64, 65):
        out.append(_case('lut8 multi S{}'.format(S), S, 3 * 126, ('multi',), policy={'rans_lut8': 1}, index_div=126, damage=S == 65,
                         why='row 1 has 257 entries and multi-boundary buckets; ragged 6-symbol tails'))
    out.append(_case('lut8 div5', 65, 20, ('eb', 4), policy={'rans_lut8': 1}, index_div=5, why='rows shorter than a chunk: every symbol on the exact path'))
    out.append(_case('lut8 div8 partial', 64, 27, ('eb', 4), policy={'rans_lut8': 1}, index_div=8, why='whole chunks; the last row holds 3 symbols'))
    out.append(_case('lut8 stride 258 falls back', 1, 16, ('shape', 4, 258), policy={'rans_lut8': 1}, index_div=4, launch=False))
    out.append(_case('lut8 1025 rows fall back', 1, 1025, ('shape', 1025, 20), policy={'rans_lut8': 1}, index_div=1, launch=False))
    # ---- explicit indexes: the four-lane decoder at more than one wave per workgroup
    for waves in (2, 4, 8):
        for S, why in ((1, 'waves past the only block return before decoding'), (70, "a wave's 16 streams straddle the end of the batch"),
                       (130, 'a third 64-stream block')):
            out.append(_case('ragged2 w{} S{}'.format(waves, S), S, 333, ('ragged', 40, 5, 600), policy={'rans_ragged2_waves': waves},
                             explicit=True, damage=(waves, S) == (2, 70), why=why))
    out.append(_case('ragged2 w4 S70 n5', 70, 5, ('ragged', 40, 5, 600), policy={'rans_ragged2_waves': 4}, explicit=True, why='shorter than a chunk'))
    out.append(_case('ragged2 w2 S70 not in LDS', 70, 333, ('ragged', 64, 600, 2400), policy={'rans_ragged2_waves': 2}, explicit=True))
    out.append(_case('ragged2 w8 S130 not in LDS', 130, 333, ('ragged', 64, 600, 2400), policy={'rans_ragged2_waves': 8}, explicit=True))
    out.append(_case('ragged2 default S1024', 1024, 16, ('ragged', 40, 5, 600), explicit=True, why='the default policy: two waves from 1 024 streams'))
    out.append(_case('ragged2 default S70', 70, 333, ('ragged', 40, 5, 600), explicit=True, why='one wave per workgroup (reached elsewhere too)'))
    # ---- explicit indexes: the one-lane ragged decoders
    out.append(_case('ragged8 in LDS', 70, 333, ('ragged', 40, 5, 600), policy={'rans_ragged2': 0}, explicit=True, damage=True))
    out.append(_case('ragged8 not in LDS', 70, 333, ('ragged', 64, 600, 2400), policy={'rans_ragged2': 0}, explicit=True))
    out.append(_case('ragged5 in LDS', 70, 333, ('ragged', 100, 5, 200), explicit=True, why='reached elsewhere too'))
    out.append(_case('ragged5 not in LDS', 70, 333, ('ragged', 80, 400, 1600), explicit=True))
    # ---- the generic decoders
    out.append(_case('generic-global 300 rows', 70, 200, ('ragged', 300, 5, 42), explicit=True, damage=True, why='more rows than the ragged decoders take'))
    out.append(_case('generic-global stride 4100', 70, 200, ('long', 4), index_div=50, why='rows too long for the LUT decoders, 16 400 entries'))
    out.append(_case('generic-lds stride 4100', 70, 100, ('long', 2), index_div=50, why='the same stride, 8 200 entries'))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

Built = collections.namedtuple('Built', 'cdfs sizes offs medians sym idx row_of streams')
_built = {}


def case_shape(c):
    """(n_cdfs, cdf_stride) of a case without building it"""
    if c.table[0] == 'shape':
        return c.table[1], c.table[2]
    b = build(c)
    return b.cdfs.shape


def _lengths(rng, kind):
    if kind[0] == 'eb':
        n = [int(rng.randint(4, 40)) for _ in range(kind[1])]
        n[0] = 6          # channel 0 is short: TIES are escapes there
        return n, None
    if kind[0] == 'eb-wide':
        n = [int(rng.randint(4, 40)) for _ in range(kind[1])]
        n[0], n[5] = 6, 299
        return n, None
    if kind[0] == 'multi':
        return [int(rng.randint(4, 40)), 256, int(rng.randint(4, 40))], {1: multi_row_pmf(rng)}
    if kind[0] == 'ragged':
        _, rows, lo, hi = kind
        n = [int(rng.randint(lo, hi)) for _ in range(rows)]
        n[rows // 2] = hi - 1          # the table's stride is the case's: hi entries
        return n, None
    if kind[0] == 'long':
        n = [int(rng.randint(4, 40)) for _ in range(kind[1])]
        n[1] = 4099
        return n, None
    raise KeyError(kind)


def build(c):
    """the case's tables, symbols, indexes and the ORACLE's stream of every image (seeded by the case's name; cached, read-only)"""
    if c.name in _built:
        return _built[c.name]
    assert c.launch, c.name
    rng = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    lengths, pmfs = _lengths(rng, c.table)
    cdfs, sizes, offs, med = make_tables(rng, lengths, pmfs)
    n_cdfs = cdfs.shape[0]
    if c.explicit:
        idx = rng.randint(0, n_cdfs, size=(c.S, c.n_sym)).astype(np.int32)
        row_of = idx
    else:
        idx = None
        row_of = np.ascontiguousarray(np.broadcast_to((np.arange(c.n_sym) // c.index_div).astype(np.int32), (c.S, c.n_sym)))
    sym = draw_symbols(rng, row_of, sizes, offs)
    if c.fused:
        assert n_cdfs == c.C and c.n_sym == c.C * c.HW and c.index_div == c.HW
        for k, p in enumerate(tie_positions(c.HW)):
            sym[:, p] = TIES[k]
    streams = [oracle_rans.encode_with_indexes(sym[i], row_of[i], cdfs, sizes, offs) for i in range(c.S)]
    for a in (cdfs, sizes, offs, med, sym, row_of):
        a.setflags(write=False)
    b = Built(cdfs, sizes, offs, med if c.fused else None, sym, idx, row_of, streams)
    _built[c.name] = b
    return b


def damage(streams):
    """the hostile streams of test_rans_decoders_terminate_on_hostile_streams on a copy: stream 3 all 0xFF (same length), stream
    9 cut to its first 16 bytes, stream 64 cut to 8 bytes (the bare initial state) -> (streams, damaged indices)"""
    out = list(streams)
    assert len(out) >= 65 and len(out[9]) > 16 and len(out[64]) > 8
    out[3] = b'\xff' * len(out[3])
    out[9] = out[9][:16]
    out[64] = out[64][:8]
    return out, [3, 9, 64]
