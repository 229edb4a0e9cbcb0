"""Shapes, qualities and contents shared by the JPEG codec tests (tests/test_jpeg_ref_cpu.py, tests/test_gpu_jpeg_codec.py).
Every content is a plane of values 0..255; a test uses it as 8-bit pixels or as the f32 values of a feature map."""
import numpy as np

GREY_SHAPES = [(1, 1), (8, 8), (13, 21), (28, 28), (64, 40)]
RGB_SHAPES = [(1, 1), (2, 2), (16, 16), (13, 21), (40, 24), (7, 35), (33, 17), (56, 56), (64, 64)]
QUALITIES = [1, 10, 50, 75, 90, 95, 100]
CONTENTS = ['random', 'smooth', 'constant', 'checker', 'isolated']


def _one_coefficient_block(u, v, amplitude):
    """8x8 samples around 128 holding one DCT basis function: a single high-frequency coefficient, every other one (nearly) zero, so
    that the zigzag scan meets a run of more than fifteen zeros in front of it."""
    k = np.arange(8)
    cu, cv = np.cos((2 * k + 1) * u * np.pi / 16), np.cos((2 * k + 1) * v * np.pi / 16)
    return 128.0 + amplitude * np.outer(cu, cv)


def plane(content, H, W, seed):
    """uint8 [H,W]"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    if content == 'random':
        p = rng.randint(0, 256, (H, W))
    elif content == 'smooth':
        p = 128 + 100 * np.sin((yy + seed) / 5.0) * np.cos((xx - seed) / 7.0)
    elif content == 'constant':
        p = np.full((H, W), 40 + 37 * (seed % 5))
    elif content == 'checker':
        p = ((yy + xx + seed) & 1) * 255
    elif content == 'isolated':
        block = _one_coefficient_block(7 - seed % 2, 6 + seed % 2, 100.0)
        p = np.tile(block, (-(-H // 8), -(-W // 8)))[:H, :W]
    else:
        raise ValueError(content)
    return np.clip(np.rint(p), 0, 255).astype(np.uint8)


def pixels(content, channels, H, W, seed=0):
    """uint8 [H,W] (channels == 1) or [3,H,W]"""
    if channels == 1:
        return plane(content, H, W, seed)
    return np.stack([plane(content, H, W, seed + 3 * c) for c in range(3)])


def features(content, C, H, W, seed=0):
    """f32 [C,H,W] with every channel group's minimum >= 0 and maximum > 0: the content's planes scaled into a feature map's range"""
    x = np.stack([plane(content, H, W, seed + 3 * c).astype(np.float32) for c in range(C)])
    scale = np.float32(0.0173) * (1 + seed % 3)
    return (x * scale + np.float32(0.25 * (seed % 2))).astype(np.float32)


def longest_zero_run(coefs, zigzag):
    """the longest run of zeros in front of a non-zero AC coefficient, over the blocks of a coefficient dict of ref_jpeg.encode"""
    best = 0
    for name in ('y', 'cb', 'cr'):
        for row in coefs.get(name, []):
            for block in row:
                run = 0
                for k in range(1, 64):
                    if block[zigzag[k]] == 0:
                        run += 1
                    else:
                        best, run = max(best, run), 0
    return best
