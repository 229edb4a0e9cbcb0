"""Sequential integer restatement of what csrc/jpeg.hip computes (include/sc2_bottleneck.h: sc2_jpeg_tensor_codec): the 8-bit
baseline JPEG process as the IJG slow-integer code runs it -- standard tables scaled by quality, 4:2:0 with the h2v2 box
downsampler, the 13-bit "islow" DCT and IDCT, one Huffman-coded scan with the Annex K tables, triangle ("fancy") chroma
upsampling -- plus the reference's normalisation of a channel group in numpy f32.  Written from the published process; no image
library is used here (tests/test_jpeg_ref_cpu.py holds it against one, byte for byte and pixel for pixel).

Everything is Python / numpy integers; blocks are visited in scan order, one after another.
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# Annex K, natural (row-major) order
LUM_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHR_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]

STATUS_NEGATIVE_MIN, STATUS_ZERO_MAX, STATUS_NOT_FINITE = 1, 2, 4
MAX_BLOCK_BITS = 22 + 63 * 26      # DC: a code of at most 11 bits + 11; AC: 63 x (16 + 10)


def quant_table(base, quality):
    """Annex K table scaled as the IJG code scales it (baseline: entries clamped to 1..255), natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * s + 50) // 100, 1), 255) for b in base]


def huff_codes(bits, vals):
    """(code, length) per symbol of a table given as counts per length and the symbols in code order."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_LUM, DC_CHR = huff_codes(DC_LUM_BITS, DC_VALS), huff_codes(DC_CHR_BITS, DC_VALS)
AC_LUM, AC_CHR = huff_codes(AC_LUM_BITS, AC_LUM_VALS), huff_codes(AC_CHR_BITS, AC_CHR_VALS)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [0] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return o


def fdct_quant(block, q):
    """8x8 samples (0..255, row-major list of 64) -> quantised coefficients in natural order."""
    w = [int(v) - 128 for v in block]
    for r in range(8):
        w[8 * r:8 * r + 8] = _fdct_1d(w[8 * r:8 * r + 8], True)
    for c in range(8):
        w[c::8] = _fdct_1d(w[c::8], False)
    out = []
    for x, qv in zip(w, q):
        d = 8 * qv
        m = (abs(x) + (d >> 1)) // d
        out.append(-m if x < 0 else m)
    return out


def _idct_1d(v, n):
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (v[0] + v[4]) << 13, (v[0] - v[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return [_descale(t10 + t3, n), _descale(t11 + t2, n), _descale(t12 + t1, n), _descale(t13 + t0, n),
            _descale(t13 - t0, n), _descale(t12 - t1, n), _descale(t11 - t2, n), _descale(t10 - t3, n)]


def dequant_idct(coef, q):
    """quantised coefficients (natural order) -> 8x8 samples 0..255."""
    w = [c * qv for c, qv in zip(coef, q)]
    for c in range(8):
        w[c::8] = _idct_1d(w[c::8], 11)
    for r in range(8):
        w[8 * r:8 * r + 8] = _idct_1d(w[8 * r:8 * r + 8], 18)
    return [min(max(v + 128, 0), 255) for v in w]


def _nbits(v):
    return abs(v).bit_length()


class _Bits(object):
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def segment(self):
        """padded with 1 bits to a whole byte; a zero byte behind every 0xFF"""
        pad = -self.n % 8
        acc, n = (self.acc << pad) | ((1 << pad) - 1), self.n + pad
        raw = acc.to_bytes(n // 8, 'big') if n else b''
        return raw.replace(b'\xff', b'\xff\x00')


def _code_block(out, coef, pred, dc_tab, ac_tab):
    diff = coef[0] - pred
    n = _nbits(diff)
    out.put(*dc_tab[n])
    if n:
        out.put((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)
    run = 0
    for k in range(1, 64):
        v = coef[ZIGZAG[k]]
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.put(*ac_tab[0xF0])
            run -= 16
        n = _nbits(v)
        out.put(*ac_tab[(run << 4) + n])
        out.put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)
        run = 0
    if run:
        out.put(*ac_tab[0x00])


def _block_of(plane, by, bx):
    return [int(v) for v in plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].reshape(-1)]


def _pad_edge(plane, rows, cols):
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode='edge')


def rgb_to_ycc(rgb):
    r, g, b = (rgb[i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def downsample(plane, blocks_x):
    """h2v2 box filter: rows padded to an even count with the last row, columns with the last pixel out to 16 x blocks_x; the bias
    alternates 1, 2 along a row; then the last output row repeated to a whole block."""
    H = plane.shape[0]
    p = _pad_edge(plane, H + (H & 1), 16 * blocks_x)
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = np.tile(np.array([1, 2], dtype=np.int64), s.shape[1] // 2)
    s = (s + bias[None, :]) >> 2
    return _pad_edge(s, -(-s.shape[0] // 8) * 8, s.shape[1])


def encode(pixels, quality):
    """pixels: uint8 [H,W] (grey) or [3,H,W] (RGB).  -> (entropy-coded segment as bytes, coefficient dict for `decode`)."""
    pixels = np.asarray(pixels)
    out = _Bits()
    if pixels.ndim == 2:
        H, W = pixels.shape
        hb, wb = -(-H // 8), -(-W // 8)
        q = quant_table(LUM_Q, quality)
        plane = _pad_edge(pixels.astype(np.int64), 8 * hb, 8 * wb)
        blocks = [[fdct_quant(_block_of(plane, by, bx), q) for bx in range(wb)] for by in range(hb)]
        pred = 0
        for by in range(hb):
            for bx in range(wb):
                _code_block(out, blocks[by][bx], pred, DC_LUM, AC_LUM)
                pred = blocks[by][bx][0]
        return out.segment(), {'mode': 'L', 'H': H, 'W': W, 'quality': quality, 'y': blocks}
    _, H, W = pixels.shape
    hb, wb, my, mx = -(-H // 8), -(-W // 8), -(-H // 16), -(-W // 16)
    ql, qc = quant_table(LUM_Q, quality), quant_table(CHR_Q, quality)
    y, cb, cr = rgb_to_ycc(pixels)
    y = _pad_edge(y, 8 * hb, 8 * wb)
    cb, cr = downsample(cb, mx), downsample(cr, mx)
    yb = [[fdct_quant(_block_of(y, by, bx), ql) for bx in range(wb)] for by in range(hb)]
    cbb = [[fdct_quant(_block_of(cb, by, bx), qc) for bx in range(mx)] for by in range(my)]
    crb = [[fdct_quant(_block_of(cr, by, bx), qc) for bx in range(mx)] for by in range(my)]
    dummy_ac = [0] * 63
    pred = [0, 0, 0]
    for m_y in range(my):
        for m_x in range(mx):
            last = None
            for k in range(4):
                by, bx = 2 * m_y + (k >> 1), 2 * m_x + (k & 1)
                # a block beyond the component's grid: no AC, the DC of the block before it in the MCU
                blk = yb[by][bx] if (by < hb and bx < wb) else [last[0]] + dummy_ac
                _code_block(out, blk, pred[0], DC_LUM, AC_LUM)
                pred[0] = blk[0]
                last = blk
            _code_block(out, cbb[m_y][m_x], pred[1], DC_CHR, AC_CHR)
            pred[1] = cbb[m_y][m_x][0]
            _code_block(out, crb[m_y][m_x], pred[2], DC_CHR, AC_CHR)
            pred[2] = crb[m_y][m_x][0]
    return out.segment(), {'mode': 'RGB', 'H': H, 'W': W, 'quality': quality, 'y': yb, 'cb': cbb, 'cr': crb}


def _plane_from_blocks(blocks, q):
    hb, wb = len(blocks), len(blocks[0])
    plane = np.zeros((8 * hb, 8 * wb), dtype=np.int64)
    for by in range(hb):
        for bx in range(wb):
            plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = np.array(dequant_idct(blocks[by][bx], q), dtype=np.int64).reshape(8, 8)
    return plane


def upsample(plane, ch, cw):
    """h2v2 of the real [ch, cw] part of a decoded chroma plane -> [2 ch, 2 cw].  More than two columns: the triangle filter (the row
    beyond an edge equals the edge row); one or two columns: every sample repeated 2 x 2."""
    p = plane[:ch, :cw]
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    out = np.zeros((2 * ch, 2 * cw), dtype=np.int64)
    for cy in range(ch):
        for v in range(2):
            far = p[max(cy - 1, 0)] if v == 0 else p[min(cy + 1, ch - 1)]
            s = 3 * p[cy] + far
            row = out[2 * cy + v]
            row[0] = (4 * s[0] + 8) >> 4
            row[2::2] = (3 * s[1:] + s[:-1] + 8) >> 4
            row[1:-1:2] = (3 * s[:-1] + s[1:] + 7) >> 4
            row[-1] = (4 * s[-1] + 7) >> 4
    return out


def decode(coefs):
    """The coefficient dict of `encode` -> uint8 [H,W] or [3,H,W]."""
    H, W, quality = coefs['H'], coefs['W'], coefs['quality']
    y = _plane_from_blocks(coefs['y'], quant_table(LUM_Q, quality))[:H, :W]
    if coefs['mode'] == 'L':
        return y.astype(np.uint8)
    qc = quant_table(CHR_Q, quality)
    ch, cw = -(-H // 2), -(-W // 2)
    cb = upsample(_plane_from_blocks(coefs['cb'], qc), ch, cw)[:H, :W] - 128
    cr = upsample(_plane_from_blocks(coefs['cr'], qc), ch, cw)[:H, :W] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b]), 0, 255).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------- the file around it
def _marker(code, payload):
    return bytes([0xFF, code]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def header(mode, H, W, quality):
    """SOI, JFIF APP0, DQT per table, SOF0, DHT per table, SOS: everything in front of the entropy-coded segment."""
    rgb = mode == 'RGB'
    out = b'\xff\xd8' + _marker(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for i, base in enumerate((LUM_Q, CHR_Q) if rgb else (LUM_Q,)):
        q = quant_table(base, quality)
        out += _marker(0xDB, bytes([i]) + bytes(q[ZIGZAG[k]] for k in range(64)))
    comps = b'\x01\x22\x00\x02\x11\x01\x03\x11\x01' if rgb else b'\x01\x11\x00'
    out += _marker(0xC0, b'\x08' + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes([3 if rgb else 1]) + comps)
    tables = [(0x00, DC_LUM_BITS, DC_VALS), (0x10, AC_LUM_BITS, AC_LUM_VALS)]
    if rgb:
        tables += [(0x01, DC_CHR_BITS, DC_VALS), (0x11, AC_CHR_BITS, AC_CHR_VALS)]
    for ident, bits, vals in tables:
        out += _marker(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    scan = b'\x03\x01\x00\x02\x11\x03\x11' if rgb else b'\x01\x01\x00'
    return out + _marker(0xDA, scan + b'\x00\x3f\x00')


def file_bytes(pixels, quality):
    pixels = np.asarray(pixels)
    segment, _ = encode(pixels, quality)
    mode = 'L' if pixels.ndim == 2 else 'RGB'
    return header(mode, pixels.shape[-2], pixels.shape[-1], quality) + segment + b'\xff\xd9'


def max_bytes(mode, H, W):
    """sc2_jpeg_max_bytes: every scan block at its longest code, every byte stuffed."""
    blocks = 6 * (-(-H // 16)) * (-(-W // 16)) if mode == 'RGB' else (-(-H // 8)) * (-(-W // 8))
    return 2 * ((blocks * MAX_BLOCK_BITS + 7) // 8)


# --------------------------------------------------------------------------------------------------------- the tensor module
def channel_groups(C):
    """[(first channel, channel count)]: threes, a remainder of one as one grey image, of two as two grey images."""
    groups = [(3 * g, 3) for g in range(C // 3)]
    return groups + [(3 * (C // 3) + i, 1) for i in range(C % 3)]


def group_status(group):
    g = np.asarray(group, dtype=np.float32)
    low, high = g.min(), g.max()
    if not np.isfinite(g).all():
        return STATUS_NOT_FINITE
    return (STATUS_NEGATIVE_MIN if low < 0 else 0) | (STATUS_ZERO_MAX if not high > 0 else 0)


def normalise(group):
    """f32 [n,H,W] -> (uint8 pixels, low, high): p = u8(trunc(((v - low) / high) * 255)), three f32 operations."""
    g = np.asarray(group, dtype=np.float32)
    low, high = g.min(), g.max()
    with np.errstate(all='ignore'):
        p = ((g - low) / high) * np.float32(255.0)
    return p.astype(np.uint8), np.float32(low), np.float32(high)


def denormalise(pixels, low, high):
    return (pixels.astype(np.float32) / np.float32(255.0)) * np.float32(high) + np.float32(low)


def tensor_codec(x, quality):
    """f32 [C,H,W] -> (reconstruction f32 [C,H,W], [segment bytes per image], [(low, high)], [status]).  An image whose status is
    not 0 has an empty segment and a zero reconstruction."""
    x = np.asarray(x, dtype=np.float32)
    recon = np.zeros_like(x)
    segments, extrema, status = [], [], []
    for c0, n in channel_groups(x.shape[0]):
        group = x[c0:c0 + n]
        st = group_status(group)
        status.append(st)
        extrema.append((np.float32(group.min()), np.float32(group.max())))
        if st:
            segments.append(b'')
            continue
        p, low, high = normalise(group)
        seg, coefs = encode(p if n == 3 else p[0], quality)
        d = decode(coefs)
        recon[c0:c0 + n] = denormalise(d if n == 3 else d[None], low, high)
        segments.append(seg)
    return recon, segments, extrema, status


def file_size(segments, H, W, quality, side_info):
    """the module's reported size of one sample: header + segment + EOI per image, plus the pickled extrema lists"""
    total = side_info
    for seg, n in segments:
        total += len(header('RGB' if n == 3 else 'L', H, W, quality)) + len(seg) + 2
    return total
