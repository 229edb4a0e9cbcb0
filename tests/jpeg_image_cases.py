"""Inputs shared by the tests of the JPEG input-compression kernels (tests/test_jpeg_image_ref_cpu.py,
tests/test_gpu_jpeg_image_codec.py): 8-bit images built deterministically with numpy -- no image library here --, the shapes at which
each mechanism of csrc/jpeg_image.hip can go wrong, and the reference results of tests/ref_jpeg.py, computed once per case and shared."""
import numpy as np

import ref_jpeg as RJ

MAX_SIDE = 2048          # SC2_JPEG_IMAGE_MAX_SIDE
CHUNK_BLOCKS = 128       # SC2_JPEG_IMAGE_CHUNK_BLOCKS (tests/test_jpeg_image_codec_cpu.py holds both against the library's constants)
# one MCU row whose scan has three whole chunks of the entropy pass and a remainder
CHUNKED_MCUS = 3 * CHUNK_BLOCKS // 6 + 1
assert 6 * CHUNKED_MCUS > 3 * CHUNK_BLOCKS and (6 * CHUNKED_MCUS) % CHUNK_BLOCKS

# (channels, H, W, content, quality)
CASES = [
    (3, 1, 1, 'noise', 75),
    (3, 8, 8, 'gradient', 90),
    (3, 16, 16, 'noise', 50),                         # one MCU
    (3, 17, 17, 'gradient', 75),                      # dummy Y blocks, odd chroma edges
    (3, 15, 33, 'noise', 90),
    (3, 3, 5, 'noise', 100),                          # a chroma plane of two columns: no triangle filter
    (3, 2, 4, 'gradient', 50),
    (3, 65, 64, 'gradient', 50),                      # the first sizes past the on-chip kernel's limit
    (3, 64, 65, 'blocks', 100),                       # DC differences of magnitude category 11
    (3, 40, 24, 'c137', 1),                           # three MCU rows: context rows both ways
    (3, 47, 49, 'noise', 100),                        # stuffed bytes
    (3, 24, 40, 'zero', 90),
    (3, 33, 17, 'white', 1),
    (3, 16, MAX_SIDE, 'gradient', 75),                # every column chunk
    (3, 1333, 16, 'gradient', 90),                    # many strips
    (3, 13, 16 * CHUNKED_MCUS - 5, 'noise', 50),      # more than two entropy chunks and a remainder
    (3, 97, 131, 'gradient', 90),
    (3, 16, 225, 'noise', 95),
    (3, 224, 224, 'gradient', 75),                    # the classifier's input size
    (1, 1, 1, 'c137', 75),
    (1, 17, 17, 'noise', 100),
    (1, 47, 49, 'blocks', 100),
    (1, 100, 75, 'gradient', 80),
    (1, 8, 1344, 'gradient', 50),                     # grey column chunks
    (1, 150, 130, 'noise', 90),                       # grey: two column chunks in every block row, three entropy chunks
]


def case_id(case):
    return '{}x{}x{}-{}-q{}'.format(*case)


def pixels(C, H, W, content, seed=0):
    """uint8 [C,H,W]"""
    rng = np.random.RandomState(1000 * seed + 7 * H + W + C)
    yy, xx = np.mgrid[0:H, 0:W]
    if content == 'noise':
        p = rng.randint(0, 256, (C, H, W))
    elif content in ('zero', 'white', 'c137'):
        p = np.full((C, H, W), {'zero': 0, 'white': 255, 'c137': 137}[content])
    elif content == 'gradient':        # natural-looking: a smooth gradient plus noise
        p = np.stack([30 + 40 * c + (150 - 30 * c) * xx / max(W - 1, 1) + (40 + 20 * c) * yy / max(H - 1, 1) for c in range(C)])
        p = p + rng.normal(0.0, 6.0, (C, H, W))
    elif content == 'blocks':          # all-0 and all-255 blocks in turn
        p = np.broadcast_to((((yy >> 3) + (xx >> 3)) & 1) * 255, (C, H, W))
    else:
        raise ValueError(content)
    return np.clip(np.rint(p), 0, 255).astype(np.uint8)


def case_pixels(case, seed=0):
    C, H, W, content, _ = case
    return pixels(C, H, W, content, seed)


_REF = {}


def reference(arr, quality):
    """uint8 [C,H,W] -> (segment bytes, coefficient dict, decoded uint8 [C,H,W], file size), once per input."""
    key = (arr.shape, quality, arr.tobytes())
    if key not in _REF:
        plain = arr[0] if arr.shape[0] == 1 else arr
        segment, coefs = RJ.encode(plain, quality)
        decoded = RJ.decode(coefs)
        decoded = decoded[None] if arr.shape[0] == 1 else decoded
        size = len(RJ.header('L' if arr.shape[0] == 1 else 'RGB', arr.shape[1], arr.shape[2], quality)) + len(segment) + 2
        _REF[key] = (segment, coefs, decoded, size)
    return _REF[key]


def scan_blocks(C, H, W):
    return 6 * (-(-H // 16)) * (-(-W // 16)) if C == 3 else (-(-H // 8)) * (-(-W // 8))
