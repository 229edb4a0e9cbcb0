"""CPU: the reference the JPEG input-compression kernels are held to (tests/ref_jpeg.py, size-generic) against Pillow at the sizes of
tests/jpeg_image_cases.py -- file bytes and decoded pixels, no tolerance --, and the conditions those inputs have to meet so that
the GPU tests reach every mechanism of csrc/jpeg_image.hip (checked on the reference alone)."""
from io import BytesIO

import numpy as np
import pytest

import jpeg_image_cases as IC
import ref_jpeg as RJ

PIL_CASES = [c for c in IC.CASES if c[1] * c[2] <= 224 * 224]


def test_the_sizes_checked_by_hand_are_cases():
    for wanted in ((3, 97, 131, 90), (3, 224, 224, 75), (3, 65, 64, 50), (3, 16, 225, 95), (1, 100, 75, 80)):
        assert any((c[0], c[1], c[2], c[4]) == wanted for c in PIL_CASES), wanted


@pytest.mark.parametrize('case', PIL_CASES, ids=IC.case_id)
def test_reference_equals_pillow(case):
    Image = pytest.importorskip('PIL.Image')
    C, H, W, _, quality = case
    arr = IC.case_pixels(case)
    segment, _, decoded, size = IC.reference(arr, quality)
    img = Image.fromarray(arr[0] if C == 1 else np.ascontiguousarray(arr.transpose(1, 2, 0)))
    assert img.mode == ('L' if C == 1 else 'RGB') and img.size == (W, H)
    coded = BytesIO()
    img.save(coded, format='JPEG', quality=quality)
    mine = RJ.header(img.mode, H, W, quality) + segment + b'\xff\xd9'
    assert len(mine) == size
    assert coded.getvalue() == mine
    theirs = np.asarray(Image.open(BytesIO(coded.getvalue())))
    theirs = theirs[None] if C == 1 else theirs.transpose(2, 0, 1)
    assert theirs.shape == decoded.shape and (theirs == decoded).all()


def test_a_case_has_ten_stuffed_bytes():
    assert max(IC.reference(IC.case_pixels(c), c[4])[0].count(b'\xff\x00') for c in IC.CASES if c[3] == 'noise' and c[4] == 100) >= 10


def test_a_case_has_dummy_luma_blocks():
    """an MCU whose four Y blocks are not all inside the block grid"""
    assert any(c[0] == 3 and (-(-c[1] // 8) % 2 or -(-c[2] // 8) % 2) for c in IC.CASES)
    case = next(c for c in IC.CASES if c[:3] == (3, 17, 17))
    coefs = IC.reference(IC.case_pixels(case), case[4])[1]
    assert len(coefs['y']) == 3 and len(coefs['cb']) == 2          # three block rows of luma in two MCU rows


def test_a_case_spans_more_than_two_entropy_chunks(S):
    assert (IC.CHUNK_BLOCKS, IC.MAX_SIDE) == (S.hip.JPEG_IMAGE_CHUNK_BLOCKS, S.hip.JPEG_IMAGE_MAX_SIDE)
    counts = [IC.scan_blocks(*c[:3]) for c in IC.CASES]
    assert max(counts) > 2 * IC.CHUNK_BLOCKS
    assert any(n > 3 * IC.CHUNK_BLOCKS and n % IC.CHUNK_BLOCKS for n in counts)      # whole chunks and a remainder
    assert any(c[0] == 1 and IC.scan_blocks(*c[:3]) > 2 * IC.CHUNK_BLOCKS for c in IC.CASES)


def _scan_order_dc_differences(coefs):
    """the DC differences the scan codes: every block against the block before it of its component in scan order (ref_jpeg.encode)"""
    if coefs['mode'] == 'L':
        dcs = [blk[0] for row in coefs['y'] for blk in row]
        return [b - a for a, b in zip([0] + dcs, dcs)]
    hb, wb, diffs, pred = len(coefs['y']), len(coefs['y'][0]), [], [0, 0, 0]
    for m_y in range(len(coefs['cb'])):
        for m_x in range(len(coefs['cb'][0])):
            last = None
            for k in range(4):
                by, bx = 2 * m_y + (k >> 1), 2 * m_x + (k & 1)
                last = coefs['y'][by][bx][0] if (by < hb and bx < wb) else last      # a dummy block: the DC before it in the MCU
                diffs.append(last - pred[0])
                pred[0] = last
            for comp, name in ((1, 'cb'), (2, 'cr')):
                diffs.append(coefs[name][m_y][m_x][0] - pred[comp])
                pred[comp] = coefs[name][m_y][m_x][0]
    return diffs


def test_a_case_has_a_dc_difference_of_category_eleven():
    for case in (c for c in IC.CASES if c[3] == 'blocks'):      # the RGB case and the grey one
        coefs = IC.reference(IC.case_pixels(case), case[4])[1]
        assert max(abs(d).bit_length() for d in _scan_order_dc_differences(coefs)) == 11, case
