"""The part of a baseline JPEG file that does not depend on the pixels: SOI, JFIF APP0, the quantisation tables (Annex K scaled by
quality, one DQT each), SOF0, the four Annex K Huffman tables (one DHT each), SOS -- as the IJG library behind Pillow writes it for
`Image.save(format='JPEG', quality=q)` of an 8-bit grey or RGB image (4:2:0).  `csrc/jpeg.hip` produces the entropy-coded segment on the
device; a file is `header + segment + EOI`, so the size `transforms.PILTensorModule` reports needs only this header's length.
Host code, a few hundred bytes per (mode, H, W, quality), built once per key.
"""
import functools

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
LUM_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHR_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
DC_LUM_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_CHR_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
DC_VALS = tuple(range(12))
AC_LUM_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)
AC_CHR_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)
AC_LUM_VALS = bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546474849'
    '4a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5'
    'c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')
AC_CHR_VALS = bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748'
    '494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3'
    'c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')


def quant_table(base, quality):
    """Annex K table at `quality` (1..100), entries clamped to 1..255 (baseline), natural order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * scale + 50) // 100, 1), 255) for b in base]


def _marker(code, payload):
    return bytes((0xFF, code)) + (len(payload) + 2).to_bytes(2, 'big') + payload


@functools.lru_cache(maxsize=None)
def header(mode, height, width, quality):
    """mode 'L' or 'RGB' -> the bytes in front of the entropy-coded segment."""
    assert mode in ('L', 'RGB') and 1 <= height <= 65535 and 1 <= width <= 65535 and 1 <= quality <= 100
    rgb = mode == 'RGB'
    out = b'\xff\xd8' + _marker(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for ident, base in enumerate((LUM_Q, CHR_Q) if rgb else (LUM_Q,)):
        table = quant_table(base, quality)
        out += _marker(0xDB, bytes((ident,)) + bytes(table[k] for k in ZIGZAG))
    components = b'\x01\x22\x00\x02\x11\x01\x03\x11\x01' if rgb else b'\x01\x11\x00'
    out += _marker(0xC0, b'\x08' + height.to_bytes(2, 'big') + width.to_bytes(2, 'big') + bytes((3 if rgb else 1,)) + components)
    tables = [(0x00, DC_LUM_BITS, DC_VALS), (0x10, AC_LUM_BITS, AC_LUM_VALS)]
    if rgb:
        tables += [(0x01, DC_CHR_BITS, DC_VALS), (0x11, AC_CHR_BITS, AC_CHR_VALS)]
    for ident, bits, vals in tables:
        out += _marker(0xC4, bytes((ident,)) + bytes(bits) + bytes(vals))
    return out + _marker(0xDA, (b'\x03\x01\x00\x02\x11\x03\x11' if rgb else b'\x01\x01\x00') + b'\x00\x3f\x00')


@functools.lru_cache(maxsize=None)
def checked_header_bytes(mode, height, width, quality):
    """len(header(...)) after holding the header against what the installed Pillow writes for an image of that mode and size (the codec
    library could be built with other defaults: then the reported sizes would not be the host path's, and this raises).  Without
    Pillow there is nothing to compare with: the length as built."""
    mine = header(mode, height, width, quality)
    try:
        from PIL import Image
    except ImportError:
        return len(mine)
    from io import BytesIO
    coded = BytesIO()
    Image.new(mode, (width, height)).save(coded, format='JPEG', quality=quality)
    theirs = coded.getvalue()
    if theirs[:len(mine)] != mine:
        raise RuntimeError('jpeg_format.header({!r}, {}, {}, {}) differs from the header Pillow writes'.format(mode, height, width, quality))
    return len(mine)
