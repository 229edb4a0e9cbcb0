"""The weight streams of the f32 and split-bf16 encoder convolutions, entry by entry against the layout formulas of
include/sc2_bottleneck.h (sc2_conv2d_f32_fwd / sc2_conv2d_split_fwd: w_frag).  CPU tensors, the library loaded for the chunk widths.

Plain index loops: nothing here reuses the packers' reshape / permute."""
import numpy as np
import pytest
import torch

# (Cout, Cin, KH, KW): chunk widths 32 / 48 / 96 / 2 x 96; K = 100, 72, 48, 36 (cin padded to a multiple of 4): not all multiples
# of 16, none but 48 a multiple of 16, none a multiple of 32; Cin 3 carries a zero fourth channel
SHAPES = [(24, 3, 5, 5), (100, 8, 3, 3), (48, 12, 2, 2), (96, 3, 3, 3)]
CHUNK = {24: 32, 48: 48, 96: 96, 100: 96}


def _weight(shape):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(shape, generator=g)


def _padded_matrix(w, rows, kpad):
    """W[row][k], k = (kh * KW + kw) * cin_pad + ci; zero beyond Cout, beyond Cin inside a tap and beyond K."""
    Cout, Cin, KH, KW = w.shape
    cin_pad = (Cin + 3) // 4 * 4
    m = np.zeros((rows, kpad), dtype=np.float32)
    wn = w.numpy()
    for co in range(Cout):
        for kh in range(KH):
            for kw in range(KW):
                for ci in range(Cin):
                    m[co, (kh * KW + kw) * cin_pad + ci] = wn[co, ci, kh, kw]
    return m, KH * KW * cin_pad


@pytest.mark.parametrize('shape', SHAPES)
def test_pack_conv_f32_layout(S, shape):
    w = _weight(shape)
    cc = int(S.hip.lib().sc2_conv_f32_chunk_channels(shape[0]))
    assert cc == CHUNK[shape[0]]
    chunks, NT = (shape[0] + cc - 1) // cc, cc // 16
    K = shape[2] * shape[3] * ((shape[1] + 3) // 4 * 4)
    steps = (K + 15) // 16
    m, k_real = _padded_matrix(w, chunks * cc, steps * 16)
    assert k_real == K
    got = S.hip.pack_conv_f32(w)
    assert got.dtype == torch.float32 and got.is_contiguous() and got.numel() == chunks * steps * NT * 64 * 4
    g = got.numpy().reshape(chunks, steps, NT, 64, 4)
    for ch in range(chunks):
        for s in range(steps):
            for nt in range(NT):
                for lane in range(64):
                    q, r = lane >> 4, lane & 15
                    for j in range(4):
                        row, k = ch * cc + nt * 16 + r, 16 * s + 4 * q + j
                        want = m[row, k]
                        assert g[ch, s, nt, lane, j] == want, (ch, s, nt, lane, j)
                        if row >= shape[0] or k >= K:
                            assert want == 0.0


@pytest.mark.parametrize('ns', [2, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_pack_conv_split_layout_and_parts(S, shape, ns):
    w = _weight(shape)
    cc = int(S.hip.lib().sc2_conv_split_chunk_channels(shape[0]))
    assert cc == CHUNK[shape[0]]
    chunks, NT = (shape[0] + cc - 1) // cc, cc // 16
    K = shape[2] * shape[3] * ((shape[1] + 3) // 4 * 4)
    steps = (K + 31) // 32
    m, _ = _padded_matrix(w, chunks * cc, steps * 32)
    parts = [p.float().numpy() for p in S.hip.split_bf16(torch.from_numpy(m), ns)]
    got = S.hip.pack_conv_split(w, ns)
    assert got.dtype == torch.bfloat16 and got.is_contiguous() and got.numel() == chunks * steps * ns * NT * 64 * 8
    g = got.float().numpy().reshape(chunks, steps, ns, NT, 64, 8)
    total = np.zeros(m.shape, dtype=np.float64)
    seen = np.zeros(m.shape, dtype=np.int32)
    for ch in range(chunks):
        for s in range(steps):
            for nt in range(NT):
                for lane in range(64):
                    q, r = lane >> 4, lane & 15
                    for j in range(8):
                        row, k = ch * cc + nt * 16 + r, 32 * s + 16 * (j >> 2) + 4 * q + (j & 3)
                        for p in range(ns):
                            v = g[ch, s, p, nt, lane, j]
                            assert v == parts[p][row, k], (ch, s, p, nt, lane, j)
                            if row >= shape[0] or k >= K:
                                assert v == 0.0
                            total[row, k] += float(v)
                        seen[row, k] += 1
    assert (seen == 1).all()          # the stream holds every element of the padded matrix exactly once
    # the parts sum back to the weight.  ns = 3: three bf16 parts hold 3 x 8 = 24 significand bits, all of an f32 (standard-normal
    # weights: nothing near underflow) -- exact.  ns = 2: two round-to-nearest steps of 2^-9 each leave at most 2^-18 |w|; the
    # bound 2^-16 |w| leaves two bits.
    err = np.abs(total - m.astype(np.float64))
    if ns == 3:
        assert (err == 0.0).all(), err.max()
    else:
        assert (err <= 2.0 ** -16 * np.abs(m.astype(np.float64))).all(), (err / np.maximum(np.abs(m), 1e-30)).max()
